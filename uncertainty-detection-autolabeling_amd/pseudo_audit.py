"""The pseudo-label audit of the reference's SSL utilities on the device: how the STAC teacher's pseudo labels (`pseudo_labels.py`)
compare with the ground truth, and the two methods built on that comparison.

The reference's `Parent_SSL.extract_pseudo_gt_data` (src/ssl_utils/parent.py:1648-1813, `_percls_analysis` :1567-1646) builds,
per image, the ground-truth x pseudo-label IoU matrix in Python, decides which pseudo label covers which ground-truth row,
allocates one row to every covering label and counts missing and extra detections.  Here the matrix work of all images is ONE
device call (C entry point uda_pseudo_audit_np, csrc/kernels_audit.hip; the contract is in include/uda_hip.h and DESIGN 19);
classes, tallies and text stay on the host, in the reference's numpy statements.

  read_kitti_annotations / read_bdd_annotations   the reference's readers (:1226-1301): a list of {"class", "bbox"} per image
  audit_np                                        lists of per-image boxes -> the raw arrays of the device call
  audit_pseudo_labels                             -> PseudoAudit: the reference's members under their names, `merge`, `totals`,
                                                  `percls`, `summary` (the text of print_data)
  corrected_pseudo                                ThreeDproblem.corrected_pseudo (3d.py:80-255) as index decisions per image;
                                                  the files are writers.write_kitti_corrected_pseudo / write_bdd_corrected_pseudo
  corrected_arrays                                the corrected set as arrays, to audit it again without a file round-trip
  pls_scores / pls_select                         Advanced_Pseudo_Labels._pls (pls.py:167-218): S_i, C_i, D_i and the
                                                  top / bot / rand selection; host numpy

Not built: the two 1000 x 2000 heat maps (:1676-1677, 1786-1795; filled and never read), the plots, the `stac_command` strings and
the folder naming, and a variant on a handle's resident detections - the final pseudo-label set exists only after
`PseudoLabelSet.finalize`'s dataset-wide normalisation, so the audit takes host arrays.
"""
import contextlib
import warnings

import numpy as np

from . import capi

DET_EXTRA, GT_NOMATCH = capi.AUDIT_DET_EXTRA, capi.AUDIT_GT_NOMATCH
MAX_G, MAX_D, MAX_B = capi.AUDIT_MAX_G, capi.AUDIT_MAX_D, capi.AUDIT_MAX_B
# ThreeDproblem.__init__ (3d.py:48-78): the six corrections and the switches each one sets
METHODS = {"nomd": dict(remove_imgs_with_mds=True), "nofd": dict(remove_fds=True),
           "nomdfd": dict(remove_imgs_with_mds=True, remove_fds=True), "fixmd": dict(add_mds=True),
           "highprec": dict(high_precision=True), "nonoise": dict(remove_noise=True)}
FLAGS = ("remove_imgs_with_mds", "remove_fds", "remove_noise", "add_mds", "high_precision")
_ROW_KEYS = (("gt_max_iou", np.float64), ("gt_best_det", np.int32), ("gt_alloc_det", np.int32), ("gt_flags", np.uint8))
_DET_KEYS = (("det_max_iou", np.float64), ("det_best_gt", np.int32), ("det_alloc_gt", np.int32), ("det_alloc_miou", np.float64),
             ("det_alloc_pair_iou", np.float64), ("det_flags", np.uint8))


def read_kitti_annotations(path, used_classes):
    """Parent_SSL._read_kitti_annotations (:1226-1254): the lines of a KITTI label file whose first word is a used class, as
    {"class", "bbox": columns 4..7 as floats}."""
    objects = []
    with open(path, "r") as f:
        for line in f.readlines():
            parts = line.strip().split(" ")
            if len(parts) > 0 and parts[0] in used_classes:
                objects.append({"class": parts[0], "bbox": [float(parts[4]), float(parts[5]), float(parts[6]), float(parts[7])]})
    return objects


def read_bdd_annotations(items, name, used_classes):
    """Parent_SSL._read_bdd100k_annotations (:1256-1301) on loaded json `items`: the labels of image `name` whose category is a
    used class, as {"class", "bbox": [y1, x1, y2, x2] as floats}."""
    names = np.asarray([item["name"] for item in items])
    hit = np.where(names == name)[0]
    if len(hit) == 0:
        raise ValueError("pseudo audit: image %r is not among the %d items" % (name, len(items)))
    objects = []
    for obj in items[hit[0]]["labels"]:
        if obj["category"] in used_classes:
            b = obj["box2d"]
            objects.append({"class": obj["category"], "bbox": [float(b["y1"]), float(b["x1"]), float(b["y2"]), float(b["x2"])]})
    return objects


def _flat(boxes_per_image, what):
    arrays = [np.asarray(b, np.float64).reshape(-1, 4) for b in boxes_per_image]
    off = np.zeros(len(arrays) + 1, np.int64)
    np.cumsum([len(a) for a in arrays], out=off[1:])
    flat = np.ascontiguousarray(np.concatenate(arrays) if arrays else np.zeros((0, 4)), np.float64)
    if not np.isfinite(flat).all():
        bad = int(np.searchsorted(off, np.where(~np.isfinite(flat).all(axis=1))[0][0], side="right") - 1)
        raise ValueError("pseudo audit: the %s boxes of image %d are not finite" % (what, bad))
    return flat, off


def audit_np(gt_boxes, det_boxes, gt_iou_thr=0.5, device=0):
    """gt_boxes / det_boxes: one [*, 4] array (or list of boxes) per image -> the dict of the flat arrays of uda_pseudo_audit_np
    (per row, per label, n_matches per image) with gt_off / det_off."""
    gt_boxes, det_boxes = list(gt_boxes), list(det_boxes)
    if len(gt_boxes) != len(det_boxes):
        raise ValueError("pseudo audit: ground truth of %d images, pseudo labels of %d" % (len(gt_boxes), len(det_boxes)))
    if not np.isfinite(float(gt_iou_thr)):
        raise ValueError("pseudo audit: gt_iou_thr must be finite, got %r" % (gt_iou_thr,))
    B = len(gt_boxes)
    if B < 1 or B > MAX_B:
        raise ValueError("pseudo audit: %d images in one call, 1..%d are taken" % (B, MAX_B))
    gt, gt_off = _flat(gt_boxes, "ground-truth")
    det, det_off = _flat(det_boxes, "pseudo-label")
    res = {k: np.zeros(len(gt), dt) for k, dt in _ROW_KEYS}
    res.update({k: np.zeros(len(det), dt) for k, dt in _DET_KEYS})
    res["n_matches"] = np.zeros(B, np.int32)
    lib = capi.load()
    rc = lib.uda_pseudo_audit_np(int(device), B, gt.ctypes.data, gt_off.ctypes.data, det.ctypes.data, det_off.ctypes.data,
                                 float(gt_iou_thr), *[res[k].ctypes.data for k, _ in _ROW_KEYS + _DET_KEYS], res["n_matches"].ctypes.data)
    capi.check(lib, None, rc, "uda_pseudo_audit_np")
    res["gt_off"], res["det_off"] = gt_off, det_off
    return res


def _split(image):
    """An image's objects: the readers' list of {"class", "bbox"} or a (boxes, classes) pair -> (list of boxes, array of classes)."""
    if isinstance(image, tuple) and len(image) == 2:
        boxes, classes = image
        return [list(map(float, b)) for b in np.asarray(boxes, np.float64).reshape(-1, 4)], np.asarray(list(classes))
    return [o["bbox"] for o in image], np.asarray([o["class"] for o in image])


class PseudoAudit:
    """The audit of a list of images, in the reference's members (parent.py:1656-1799), one entry per image:

      n_gts_perim, n_pred_perim, n_gt_matches, n_extra_detections   counts
      matched_preds, nomatch_preds     the labels that cover a row (ascending) and the others (:1736-1742)
      matched_gt                       the row each matched prediction took (:1744-1752)
      allocated_dets                   {"gt" | "pseudo": {"class", "box"}} of the allocated pairs (:1773-1784)
      collect_gt_boxes / _classes, collect_pseudo_boxes / _classes
      gt_max_iou, gt_best_det          np.max / np.argmax of the rows of perim_ious (in place of the matrices themselves)
      det_max_iou, det_best_gt         the same per label (3d.py:150-152)
      mious, alloc_pair_iou, macc      per allocated pair: np.max of the mutated row (:1763-1765), the pair's IoU (:1572-1581),
                                       whether the classes agree (:1754-1762)
      extra_dets, nomatch_gts          the by-value index lists of _percls_analysis (:1614-1636)
    `n_missing_dets` is the array of :1797-1799."""

    _LISTS = ("names", "n_gts_perim", "n_pred_perim", "n_gt_matches", "n_extra_detections", "matched_preds", "nomatch_preds", "matched_gt",
              "collect_gt_boxes", "collect_gt_classes", "collect_pseudo_boxes", "collect_pseudo_classes", "gt_max_iou", "gt_best_det",
              "det_max_iou", "det_best_gt", "mious", "alloc_pair_iou", "macc", "extra_dets", "nomatch_gts")

    def __init__(self, used_classes, gt_iou_thr=0.5):
        self.used_classes, self.gt_iou_thr = list(used_classes), float(gt_iou_thr)
        for k in self._LISTS:
            setattr(self, k, [])
        self.allocated_dets = {"gt": {"class": [], "box": []}, "pseudo": {"class": [], "box": []}}

    def __len__(self):
        return len(self.n_gts_perim)

    @classmethod
    def from_arrays(cls, res, gt, dets, used_classes, gt_iou_thr=0.5, names=None):
        self = cls(used_classes, gt_iou_thr)
        n = len(gt)
        self.names = list(range(n)) if names is None else list(names)
        if len(self.names) != n:
            raise ValueError("pseudo audit: %d names for %d images" % (len(self.names), n))
        for b in range(n):
            g0, g1, d0, d1 = int(res["gt_off"][b]), int(res["gt_off"][b + 1]), int(res["det_off"][b]), int(res["det_off"][b + 1])
            gt_boxes, gt_classes = gt[b]
            det_boxes, det_classes = dets[b]
            alloc = res["det_alloc_gt"][d0:d1]
            matched_pred = np.where(alloc >= 0)[0]
            matched_gt = [int(r) for r in alloc[matched_pred]]
            self.n_gts_perim.append(g1 - g0)
            self.n_pred_perim.append(d1 - d0)
            self.n_gt_matches.append(int(res["n_matches"][b]))
            self.n_extra_detections.append(d1 - d0 - int(res["n_matches"][b]))
            self.matched_preds.append(matched_pred)
            self.nomatch_preds.append(np.setdiff1d(np.arange(d1 - d0), matched_pred))
            self.matched_gt.append(matched_gt)
            self.collect_gt_boxes.append(gt_boxes)
            self.collect_gt_classes.append(gt_classes)
            self.collect_pseudo_boxes.append(det_boxes)
            self.collect_pseudo_classes.append(det_classes)
            self.gt_max_iou.append(res["gt_max_iou"][g0:g1].copy())
            self.gt_best_det.append(res["gt_best_det"][g0:g1].astype(np.int64))
            self.det_max_iou.append(res["det_max_iou"][d0:d1].copy())
            self.det_best_gt.append(res["det_best_gt"][d0:d1].astype(np.int64))
            self.mious.append([res["det_alloc_miou"][d0 + i] for i in matched_pred])
            self.alloc_pair_iou.append(res["det_alloc_pair_iou"][d0:d1][matched_pred])
            self.macc.append([gt_classes[r] == det_classes[i] for r, i in zip(matched_gt, matched_pred)])
            self.extra_dets.append([int(i) for i in np.where(res["det_flags"][d0:d1] & DET_EXTRA)[0]])
            self.nomatch_gts.append([int(i) for i in np.where(res["gt_flags"][g0:g1] & GT_NOMATCH)[0]])
            self.allocated_dets["gt"]["class"].append([gt_classes[r] for r in matched_gt])
            self.allocated_dets["gt"]["box"].append([gt_boxes[r] for r in matched_gt])
            self.allocated_dets["pseudo"]["class"].append([det_classes[i] for i in matched_pred])
            self.allocated_dets["pseudo"]["box"].append([det_boxes[i] for i in matched_pred])
        return self

    def merge(self, other):
        """Appends the images of another audit (of the same classes and threshold); returns self."""
        if list(other.used_classes) != self.used_classes or other.gt_iou_thr != self.gt_iou_thr:
            raise ValueError("pseudo audit: merge of audits with different classes or thresholds")
        for k in self._LISTS:
            getattr(self, k).extend(getattr(other, k))
        for side in ("gt", "pseudo"):
            for k in ("class", "box"):
                self.allocated_dets[side][k].extend(other.allocated_dets[side][k])
        return self

    @property
    def n_missing_dets(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            return (np.asarray(self.n_gts_perim) - np.asarray(self.n_gt_matches)) / np.asarray(self.n_gts_perim)     # :1797-1799

    def totals(self):
        """The numbers of :1797-1809, by the same numpy statements in float64."""
        macc = np.concatenate([np.asarray(m, bool) for m in self.macc]) if len(self) else np.zeros(0, bool)
        mious = np.concatenate([np.asarray(m, np.float64) for m in self.mious]) if len(self) else np.zeros(0)
        with np.errstate(divide="ignore", invalid="ignore"):
            matched_gts_percent = np.round(np.sum(self.n_gt_matches) / np.sum(self.n_gts_perim) * 100, 2)
            extra_detections_percent = np.round(np.sum(np.sum(self.n_extra_detections)) / np.sum(self.n_pred_perim) * 100, 2)
            m_macc = np.round(np.sum(macc) / len(macc) * 100, 2) if len(macc) else np.float64("nan")
            m_miou = np.round(np.mean(mious) * 100, 2) if len(mious) else np.float64("nan")
        return dict(n_gts=np.sum(self.n_gts_perim), n_preds=np.sum(self.n_pred_perim), found_gts=np.sum(self.n_gt_matches),
                    matched_gts_percent=matched_gts_percent, missing_percent=np.round(100 - matched_gts_percent, 2),
                    n_extra=np.sum(self.n_extra_detections), extra_detections_percent=extra_detections_percent, m_macc=m_macc,
                    m_miou=m_miou)

    @staticmethod
    def _cat(lists, dtype=None):
        parts = [np.asarray(c, dtype) for c in lists if len(c) > 0]
        return np.concatenate(parts) if parts else np.zeros(0, dtype or "<U1")

    def percls(self):
        """_percls_analysis (:1567-1646): per used class the mean IoU of the allocated pairs (rounded to 2), the accuracy, and the
        counts of matched labels / rows and of by-value unmatched labels / rows.  nan where no allocated row has the class."""
        gt_classes = self._cat(self.allocated_dets["gt"]["class"])
        det_classes = self._cat(self.allocated_dets["pseudo"]["class"])
        ious = self._cat(self.alloc_pair_iou, np.float64)
        perc_miou, perc_acc = [], []
        with np.errstate(divide="ignore", invalid="ignore"), _quiet_empty_mean():
            for cls in self.used_classes:
                sel = gt_classes == cls
                perc_acc.append(np.round(np.mean(gt_classes[sel] == det_classes[sel]), 2))
                perc_miou.append(np.mean(ious[sel]))
        ed = self._cat([np.asarray(c)[e] for c, e in zip(self.collect_pseudo_classes, self.extra_dets) if len(e)])
        mp = self._cat([np.asarray(c)[e] for c, e in zip(self.collect_gt_classes, self.nomatch_gts) if len(e)])
        uc = self.used_classes
        return dict(miou=dict(zip(uc, np.round(perc_miou, 2))), acc=dict(zip(uc, perc_acc)),
                    matched_dets={c: np.sum(det_classes == c) for c in uc}, matched_gt={c: np.sum(gt_classes == c) for c in uc},
                    nomatch_dets={c: np.sum(ed == c) for c in uc}, nomatch_gt={c: np.sum(mp == c) for c in uc})

    def summary(self):
        """The text of print_data (:1810-1811 and the lines _percls_analysis adds)."""
        t, p = self.totals(), self.percls()
        text = (f"number of gts: {t['n_gts']}\nnumber of preds: {t['n_preds']}\nfound gts: {t['found_gts']}, {t['matched_gts_percent']}(%), "
                f"missing {t['missing_percent']}(%)\nextra possibly false preds: {t['n_extra']}, {t['extra_detections_percent']}(%)\n"
                f"mAcc on found dets: {t['m_macc']}%\nmIoU on found dets: {t['m_miou']}%")
        text += "\n"
        text += f"mIou: {p['miou']}\n"
        text += f"Acc: {p['acc']}\n"
        text += f"Matched Dets: {p['matched_dets']}\n"
        text += f"Matched GT: {p['matched_gt']}\n"
        text += f"No Match Dets: {p['nomatch_dets']}\n"
        text += f"No Match GT: {p['nomatch_gt']}\n"
        return text


@contextlib.contextmanager
def _quiet_empty_mean():
    """np.mean of an empty selection is nan, as in the reference; its RuntimeWarning is not repeated here."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


def audit_pseudo_labels(gt, dets, used_classes, gt_iou_thr=0.5, names=None, allow_empty=False, audit=None, device=0):
    """gt / dets: per image the readers' list of {"class", "bbox"}, or a (boxes, classes) pair -> PseudoAudit.
    audit: a stand-in for `audit_np` with its signature (the host tests pass a numpy mirror).  The reference raises on an image
    without a ground-truth row (np.argmax of an empty list) or without a pseudo label (calc_iou_np indexes an empty array): so
    does this, with a ValueError naming the image, unless allow_empty - then such an image has no match, every label is extra and
    every row unmatched."""
    gt, dets = [_split(im) for im in gt], [_split(im) for im in dets]
    if len(gt) != len(dets):
        raise ValueError("pseudo audit: ground truth of %d images, pseudo labels of %d" % (len(gt), len(dets)))
    if names is not None and len(names) != len(gt):
        raise ValueError("pseudo audit: %d names for %d images" % (len(names), len(gt)))
    if not allow_empty:
        for b, ((gb, _), (db, _)) in enumerate(zip(gt, dets)):
            if len(gb) == 0 or len(db) == 0:
                raise ValueError("pseudo audit: image %r has %d ground-truth rows and %d pseudo labels; the reference raises on an "
                                 "empty side (allow_empty=True defines it)" % (b if names is None else names[b], len(gb), len(db)))
    run = audit_np if audit is None else audit
    res = run([g[0] for g in gt], [d[0] for d in dets], gt_iou_thr, device=device)
    return PseudoAudit.from_arrays(res, gt, dets, used_classes, gt_iou_thr, names)


class PseudoCorrection:
    """ThreeDproblem.corrected_pseudo's decision per image, as indices: flags (the five switches), iou_thr, and per image
    `selector` (np.unique of the best labels of the rows at or above iou_thr, 3d.py:137-140), `dropped`, `kept` (label indices, in
    order), `replacements` ([k, 2]: label, ground-truth row whose line replaces it) and `appended` (ground-truth rows added last)."""

    def __init__(self, flags, iou_thr):
        self.flags, self.iou_thr = dict(flags), iou_thr
        self.selector, self.dropped, self.kept, self.replacements, self.appended = [], [], [], [], []

    def __len__(self):
        return len(self.dropped)


def resolve_flags(method=None, **flags):
    """One of METHODS, or the switches of corrected_pseudo themselves -> the dict of all five."""
    if method is not None:
        if flags:
            raise ValueError("corrected_pseudo: give a method or flags, not both")
        if method not in METHODS:
            raise ValueError("corrected_pseudo: unknown method %r, choose among %s" % (method, tuple(METHODS)))
        flags = METHODS[method]
    unknown = [k for k in flags if k not in FLAGS]
    if unknown:
        raise ValueError("corrected_pseudo: unknown flag %r, choose among %s" % (unknown[0], FLAGS))
    return {k: bool(flags.get(k, False)) for k in FLAGS}


def corrected_pseudo(audit, method=None, **flags):
    """ThreeDproblem.corrected_pseudo (3d.py:131-160 / 179-216) on a PseudoAudit -> PseudoCorrection.  Thresholds 0.9
    (high_precision), 0.75 (remove_noise), else 0.5; remove_fds / high_precision override the noise replacement; add_mds appends
    last; remove_imgs_with_mds drops an image with n_missing_dets > 0."""
    f = resolve_flags(method, **flags)
    iou_thr = 0.9 if f["high_precision"] else 0.75 if f["remove_noise"] else 0.5
    out = PseudoCorrection(f, iou_thr)
    n_missing = audit.n_missing_dets
    for i in range(len(audit)):
        gt_selector = audit.gt_max_iou[i] >= iou_thr
        selector = np.unique(audit.gt_best_det[i][gt_selector])
        kept = np.arange(audit.n_pred_perim[i])
        repl = np.zeros((0, 2), np.int64)
        if f["remove_noise"]:
            repl = np.stack([selector, audit.det_best_gt[i][selector]], axis=1).astype(np.int64)
        if f["remove_fds"] or f["high_precision"]:
            kept, repl = selector, np.zeros((0, 2), np.int64)
        out.selector.append(selector)
        out.dropped.append(bool(f["remove_imgs_with_mds"] and n_missing[i] > 0))
        out.kept.append(kept)
        out.replacements.append(repl)
        out.appended.append(np.where(~gt_selector)[0] if f["add_mds"] else np.zeros(0, np.int64))
    return out


def corrected_arrays(audit, correction, dataset="KITTI"):
    """The corrected set as `audit_pseudo_labels` takes it: (names, gt, dets) of the images the reference would read back
    (3d.py:245-247), in the audit's order.  KITTI: a dropped image and one left without a line have no file.  BDD100K: an image
    whose selector is empty stays as it was (:189), a dropped one loses its entry.  (The 83-character cut of the KITTI `nonoise`
    files is a property of the written text and is not applied to the numbers.)"""
    if dataset not in ("KITTI", "BDD100K"):
        raise ValueError("corrected_arrays: dataset %r is neither 'KITTI' nor 'BDD100K'" % (dataset,))
    names, gt, dets = [], [], []
    for i in range(len(audit)):
        gb, gc = audit.collect_gt_boxes[i], np.asarray(audit.collect_gt_classes[i])
        boxes, classes = [list(b) for b in audit.collect_pseudo_boxes[i]], list(audit.collect_pseudo_classes[i])
        unchanged = dataset == "BDD100K" and len(correction.selector[i]) == 0
        if not unchanged:
            if correction.dropped[i]:
                continue
            for d, r in correction.replacements[i]:
                boxes[d], classes[d] = list(gb[r]), gc[r]
            if correction.flags["remove_fds"] or correction.flags["high_precision"]:
                boxes, classes = [boxes[d] for d in correction.kept[i]], [classes[d] for d in correction.kept[i]]
            boxes += [list(gb[r]) for r in correction.appended[i]]
            classes += [gc[r] for r in correction.appended[i]]
            if dataset == "KITTI" and len(boxes) == 0:
                continue
        names.append(audit.names[i])
        gt.append((gb, gc))
        dets.append((np.asarray(boxes, np.float64).reshape(-1, 4), np.asarray(classes, dtype=str) if classes else np.zeros(0, "<U1")))
    return names, gt, dets


def pls_scores(audit, scores_per_image, delta_s, beta):
    """The numbers of Advanced_Pseudo_Labels._pls (pls.py:167-204).  scores_per_image: the detection scores of every image of
    the audit, in its order; delta_s: the index of the score threshold among np.linspace(0, 1, 11) (the reference reads the
    digit from its folder name: 4 for `score_thr_04`) or that threshold itself as a float below 1."""
    if len(scores_per_image) != len(audit):
        raise ValueError("pls: scores of %d images for an audit of %d" % (len(scores_per_image), len(audit)))
    if isinstance(delta_s, float):
        delta_s = int(round(delta_s * 10))
    if not 0 <= int(delta_s) <= 10:
        raise ValueError("pls: delta_s %r is not an index into np.linspace(0, 1, 11)" % (delta_s,))
    match_score_perim = [np.asarray(s) for s in scores_per_image]
    drate = [np.asarray([np.sum(np.asarray(sp) >= i) for sp in match_score_perim]) for i in np.linspace(0, 1, 11)]
    n_det = [len(a) for a in match_score_perim]
    with np.errstate(divide="ignore", invalid="ignore"), _quiet_empty_mean():
        s_i = drate[int(delta_s)] / drate[0]
        differences = [drate[i - 1] - drate[i] for i in range(1, len(drate))]
        max_drop, mean_drop, std_drop = np.max(differences, axis=0), np.mean(differences, axis=0), np.std(differences, axis=0)
        avg_score = [np.mean(a) for a in match_score_perim]
        all_pred_classes = PseudoAudit._cat(audit.collect_pseudo_classes)
        len_perc = {c: 1 - np.sum(all_pred_classes == c) / len(all_pred_classes) for c in audit.used_classes}
        c_i = [np.mean([len_perc[c] for c in pred_classes]) for pred_classes in audit.collect_pseudo_classes]
    d_i = (1 - beta) * np.asarray(s_i) + np.asarray(c_i) * beta
    return dict(s_i=s_i, c_i=c_i, d_i=d_i, max_drop=max_drop, mean_drop=mean_drop, std_drop=std_drop, n_det=n_det,
                avg_score=avg_score, md=audit.n_missing_dets)


def pls_select(d_i, top_k, rng=None):
    """pls.py:206-218 -> (top, bot, rand) image indices.  rng: a numpy.random.RandomState (None: the global one, as the
    reference's np.random.shuffle)."""
    d_i = np.asarray(d_i)
    threshold = np.percentile(d_i, top_k * 100)
    top, bot = np.where(d_i >= threshold)[0], np.where(d_i < threshold)[0]
    rand = np.arange(len(d_i))
    (np.random if rng is None else rng).shuffle(rand)
    return top, bot, rand[: len(top)]
