"""numpy mirror of the pseudo-label audit's contract (include/uda_hip.h), written from the reference's statements
(src/ssl_utils/parent.py:1567-1813; 3d.py:150-152) and not from the kernel: per image a stored G x D matrix, np.argmax / np.max /
np.unique, the `while idx in matched_gt: ious[idx, i] = -1` loop on a MUTATED copy, and `in` / np.all for the by-value flags.
The kernel uses a closed form (no matrix, no mutation); this file does not.

  audit(gt_boxes, det_boxes, gt_iou_thr)   lists of per-image [*, 4] arrays -> the dict of flat arrays `pseudo_audit.audit_np` returns
"""
import numpy as np

from glc_ref import calc_iou

DET_EXTRA, GT_NOMATCH = 1, 1


def audit_image(gt, det, thr):
    gt, det = np.asarray(gt, np.float64).reshape(-1, 4), np.asarray(det, np.float64).reshape(-1, 4)
    G, D = len(gt), len(det)
    out = dict(gt_max_iou=np.zeros(G), gt_best_det=np.full(G, -1, np.int32), gt_alloc_det=np.full(G, -1, np.int32),
               gt_flags=np.full(G, GT_NOMATCH, np.uint8), det_max_iou=np.zeros(D), det_best_gt=np.full(D, -1, np.int32),
               det_alloc_gt=np.full(D, -1, np.int32), det_alloc_miou=np.zeros(D), det_alloc_pair_iou=np.zeros(D),
               det_flags=np.full(D, DET_EXTRA, np.uint8), n_matches=0)
    if G == 0 or D == 0:                                     # defined here, the reference raises
        return out
    ious = np.asarray([calc_iou(g, det, False) for g in gt])                           # :1732-1734
    out["gt_max_iou"], out["gt_best_det"] = np.max(ious, axis=-1), np.argmax(ious, axis=-1).astype(np.int32)
    out["det_max_iou"], out["det_best_gt"] = np.max(ious.T, axis=-1), np.argmax(ious.T, axis=-1).astype(np.int32)   # 3d.py:150-152
    matched_pred = np.unique(np.argmax(ious, axis=-1)[np.max(ious, axis=-1) >= thr])   # :1736-1738
    matched_gt = []
    for i in matched_pred:                                                             # :1744-1752
        idx = np.argmax(ious[:, i])
        while idx in matched_gt:
            ious[idx, i] = -1
            idx = np.argmax(ious[:, i])
        matched_gt.append(idx)
    mious = [np.max(ious[i]) for i in matched_gt]                                      # :1763-1765, on the mutated matrix
    out["n_matches"] = len(matched_pred)
    for i, r, m in zip(matched_pred, matched_gt, mious):
        out["det_alloc_gt"][i], out["gt_alloc_det"][r], out["det_alloc_miou"][i] = r, i, m
        out["det_alloc_pair_iou"][i] = calc_iou(gt[r], det[i:i + 1], False)[0]         # :1572-1581
    ab_det = [list(det[i]) for i in matched_pred]
    ab_gt = [list(gt[r]) for r in matched_gt]
    for d in range(D):                                                                 # :1614-1619
        out["det_flags"][d] = DET_EXTRA if list(det[d]) not in ab_det else 0
    for g in range(G):                                                                 # :1629-1636
        hit = len(ab_gt) > 0 and np.any(np.all(np.asarray(gt[g]) == np.asarray(ab_gt), axis=-1))
        out["gt_flags"][g] = 0 if hit else GT_NOMATCH
    return out


KEYS = ("gt_max_iou", "gt_best_det", "gt_alloc_det", "gt_flags", "det_max_iou", "det_best_gt", "det_alloc_gt", "det_alloc_miou",
        "det_alloc_pair_iou", "det_flags")


def audit(gt_boxes, det_boxes, gt_iou_thr=0.5, device=0):
    per = [audit_image(g, d, gt_iou_thr) for g, d in zip(gt_boxes, det_boxes)]
    res = {k: np.concatenate([p[k] for p in per]) for k in KEYS}
    res["n_matches"] = np.asarray([p["n_matches"] for p in per], np.int32)
    res["gt_off"] = np.concatenate([[0], np.cumsum([len(p["gt_flags"]) for p in per])]).astype(np.int64)
    res["det_off"] = np.concatenate([[0], np.cumsum([len(p["det_flags"]) for p in per])]).astype(np.int64)
    return res
