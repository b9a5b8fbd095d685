"""numpy mirror of the label check's contract (include/uda_hip.h; reference src/ssl_utils/glc.py:182-187, 432-436,
551, 813-834), written from the contract and not from the kernel: plain per-image numpy, the reference's own expressions
(np.argmax, np.max, np.where(...)[0][0]) on the kept detections, in both arithmetic variants.

  f32=False   float64 arrays, everything float64 - the reference's arithmetic on the literals of a prediction_data.txt
  f32=True    float32 arrays: float32 coordinate differences, float64 products, score tests in float32 - the handle's
"""
import numpy as np

MD, MISTAKES, NOISY = 1, 2, 4
GT_MISTAKE, GT_NOISY, GT_REPLACED = 1, 2, 4
DET_KEPT, DET_MISSING = 1, 2
METHOD_BITS = {"md": MD, "mistakes": MISTAKES, "noisy": NOISY}


def calc_iou(gt, boxes, f32):
    """calc_iou_np(gt [4], boxes [K, 4]) -> [K] float64 (utils_box.py:56-89)."""
    dt = np.float32 if f32 else np.float64
    gt, boxes = np.asarray(gt, dt)[None, :], np.asarray(boxes, dt).reshape(-1, 4)
    yA, xA = np.maximum(gt[:, 0], boxes[:, 0]), np.maximum(gt[:, 1], boxes[:, 1])
    yB, xB = np.minimum(gt[:, 2], boxes[:, 2]), np.minimum(gt[:, 3], boxes[:, 3])
    inter = np.maximum(dt(0), xB - xA).astype(np.float64) * np.maximum(dt(0), yB - yA).astype(np.float64)
    area_a = np.abs(gt[:, 3] - gt[:, 1]).astype(np.float64) * np.abs(gt[:, 2] - gt[:, 0]).astype(np.float64)
    area_b = np.abs(boxes[:, 3] - boxes[:, 1]).astype(np.float64) * np.abs(boxes[:, 2] - boxes[:, 0]).astype(np.float64)
    union = (area_a + area_b) - inter
    return np.divide(inter, union, out=np.zeros_like(inter), where=union != 0)


def method_mask(methods):
    return sum(METHOD_BITS[m] for m in set(methods))


def check(boxes, scores, cons_iou, gt_boxes, gt_classes, min_score, iou_consist=0.90, md_max_inter=0, md_rule="eq",
          correct_max_inter=1.0, correct_score=0.40, methods=("md", "mistakes", "noisy"), f32=False):
    """-> dict of the arrays uda_get_label_check returns, for boxes [n, M, 4], scores [n, M], cons_iou [n, M] (None for
    mistakes alone), gt_boxes [n, G, 4], gt_classes [n, G]."""
    dt = np.float32 if f32 else np.float64
    boxes, scores = np.asarray(boxes, dt), np.asarray(scores, dt)
    gt_boxes, gt_classes = np.asarray(gt_boxes, dt), np.asarray(gt_classes, dt)
    n, M = scores.shape
    G = gt_classes.shape[1]
    mask = method_mask(methods)
    out = dict(det_rank=np.full((n, G), -1, np.int32), iou=np.zeros((n, G)), gt_flags=np.zeros((n, G), np.uint8),
               gt_boxes_out=gt_boxes.astype(np.float32), det_flags=np.zeros((n, M), np.uint8), det_max_iou=np.zeros((n, M)),
               counts=np.zeros((n, 5), np.int32))
    for i in range(n):
        kept = np.where(scores[i] > dt(min_score))[0]            # the rows of prediction_data.txt, in rank order
        rows = np.where(gt_classes[i] > 0)[0]                    # the image's boxes of the used classes
        out["counts"][i, :2] = len(kept), len(rows)
        out["det_flags"][i, kept] = DET_KEPT
        if not len(kept):
            continue                                             # the image never appears in the file
        pred = boxes[i, kept]
        sc = scores[i, kept]
        ious = np.stack([calc_iou(gt_boxes[i, g], pred, f32) for g in rows]) if len(rows) else np.zeros((0, len(kept)))
        matched = np.argmax(ious, axis=-1) if len(rows) else np.zeros((0,), np.int64)
        iou_gt = np.max(ious, axis=-1) if len(rows) else np.zeros((0,))
        det_max = np.max(ious, axis=0) if len(rows) else np.zeros((len(kept),))
        out["det_rank"][i, rows] = kept[matched]
        out["iou"][i, rows] = iou_gt
        out["det_max_iou"][i, kept] = det_max
        if mask & MISTAKES:
            wrong = np.where(iou_gt == 0)[0]
            out["gt_flags"][i, rows[wrong]] |= GT_MISTAKE
            out["counts"][i, 2] = len(wrong)
        if mask & MD:
            ci = np.asarray(cons_iou[i], np.float64)[kept]
            hit = np.less_equal(det_max, md_max_inter) if md_rule == "le" else np.equal(det_max, md_max_inter)
            extra = hit * np.greater_equal(ci, iou_consist)
            out["det_flags"][i, kept[extra]] |= DET_MISSING
            out["counts"][i, 4] = int(extra.sum())
        if mask & NOISY and len(rows):
            ci = np.asarray(cons_iou[i], np.float64)[kept]
            cond = (ci[matched] > iou_consist) * (iou_gt <= correct_max_inter) * (sc[matched] >= dt(correct_score))
            out["gt_flags"][i, rows[cond]] |= GT_NOISY
            better = matched[cond]
            for k in range(len(kept)):
                if k in better:
                    g = rows[np.where(matched == k)[0][0]]
                    out["gt_boxes_out"][i, g] = pred[k].astype(np.float32)
                    out["gt_flags"][i, g] |= GT_REPLACED
                    out["counts"][i, 3] += 1
    return out

