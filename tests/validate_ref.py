"""numpy restatement of the ground-truth assignment the reference's validate and calibrate modes run on the host after
`serve` (written from utils_extra.py:44-64, utils_box.py:56-103, validate_model.py:159-202, 314-470, 706-735 and
calibrate_model.py:133-211; no text copied).  tests/golden/gt_assign_golden.npz holds what the reference's own
`gt_box_assigner` / `calc_iou_np` return for the same inputs; test_validate_host.py holds this file to it."""
import numpy as np

from consistency_ref import calc_iou_np            # utils_box.calc_iou_np, the restatement the consistency check already pins

METHODS = ("IoU", "MSE", "rank")


def mse_keys(gt_box, boxes):
    """np.mean(np.square(gt - boxes), axis=1) in float32, written out: differences, squares, ((s0 + s1) + s2) + s3 (numpy sums
    a 4-element inner axis in sequence), divided by 4."""
    d = np.asarray(gt_box, np.float32)[None, :] - np.asarray(boxes, np.float32)
    s = d * d
    return (((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]) / np.float32(4)


def iou_keys(gt_box, boxes):
    boxes = np.asarray(boxes, np.float32)
    return calc_iou_np(np.repeat(np.asarray(gt_box, np.float32)[None, :], len(boxes), 0), boxes)


def assign_one(method, gt_box, boxes, i):
    """utils_extra.gt_box_assigner for GT row i; first occurrence on ties (np.argmax / np.argmin)."""
    if method == "MSE":
        return int(np.argmin(mse_keys(gt_box, boxes)))
    if method == "IoU":
        return int(np.argmax(iou_keys(gt_box, boxes)))
    return int(i)


def kept_rows(gt_classes_i, M, keep):
    """validate: rows with class > 0 (validate_model.py:314); calibrate: rows < min(G, M) with class >= 0
    (calibrate_model.py:133-135)."""
    c = np.asarray(gt_classes_i, np.float32)
    if keep == "validate":
        return np.where(c > 0)[0]
    if keep == "calibrate":
        return np.where(c[:min(len(c), M)] >= 0)[0]
    raise ValueError(keep)


def assign(method, gt_boxes, gt_classes, boxes, keep="validate"):
    """gt_boxes [n, G, 4], gt_classes [n, G], boxes [n, M, >= 4] -> det_index [n, G] int32 (-1: not kept), iou [n, G]
    float64 (IoU of the GT box with its matched box, whatever the method), count [n] int32."""
    gt_boxes = np.asarray(gt_boxes, np.float32)
    gt_classes = np.asarray(gt_classes, np.float32)
    boxes = np.asarray(boxes, np.float32)[..., :4]
    n, G = gt_classes.shape
    M = boxes.shape[1]
    idx = np.full((n, G), -1, np.int32)
    iou = np.zeros((n, G), np.float64)
    count = np.zeros((n,), np.int32)
    for im in range(n):
        rows = kept_rows(gt_classes[im], M, keep)
        count[im] = len(rows)
        for i in rows:
            k = assign_one(method, gt_boxes[im, i], boxes[im], i)
            if k >= M:
                raise ValueError("kept ground-truth row %d beyond the %d detections" % (i, M))
            idx[im, i] = k
            iou[im, i] = calc_iou_np(gt_boxes[im, i:i + 1], boxes[im, k:k + 1])[0]
    return idx, iou, count


def unpack(params, det, probab=None, entropy=None):
    """The split `Validate._process_val_image` makes of the serve() tuple (validate_model.py:159-202): box columns 4: are
    the aleatoric and / or MC box std, class columns 1: the MC std of the logits, all through np.nan_to_num."""
    boxes, scores, classes = det[0], det[1], det[2]
    logits = det[4] if len(det) > 4 else None
    mc = bool(params.get("mc_dropout"))
    mc_box = mc and bool(params.get("mc_boxheadrate") or params.get("mc_dropoutrate"))
    la = bool(params.get("loss_attenuation"))
    out = dict(boxes=boxes[..., :4], scores=scores, classes=classes, logits=logits, probab=probab, entropy=entropy,
               albox=None, mcbox=None, mcclass=None)
    if mc_box and la:
        out["albox"], out["mcbox"] = np.nan_to_num(boxes[..., 4:8]), np.nan_to_num(boxes[..., 8:])
    elif mc_box:
        out["mcbox"] = np.nan_to_num(boxes[..., 4:])
    elif la:
        out["albox"] = np.nan_to_num(boxes[..., 4:])
    if classes.ndim == 3:
        out["mcclass"] = np.nan_to_num(classes[..., 1:])
        out["classes"] = classes[..., 0]
    return out


COLUMNS = ("scores", "boxes", "classes", "logits", "probab", "entropy", "mcclass", "mcbox", "albox")


def gather(params, det, det_index, gt_boxes, gt_classes, probab=None, entropy=None, keep="validate"):
    """The matched rows in (image, GT row) order - the order the reference appends in: every column of `unpack` at the
    matched rank, plus gt_boxes / gt_classes (calibrate reports class - 1, calibrate_model.py:137), image and gt_row."""
    un = unpack(params, det, probab, entropy)
    im, row = np.nonzero(np.asarray(det_index) >= 0)
    k = np.asarray(det_index)[im, row]
    out = {c: (None if un[c] is None else np.asarray(un[c])[im, k]) for c in COLUMNS}
    out["gt_boxes"] = np.asarray(gt_boxes, np.float32)[im, row]
    cls = np.asarray(gt_classes, np.float32)[im, row]
    out["gt_classes"] = cls - np.float32(1) if keep == "calibrate" else cls
    out["image"], out["gt_row"] = im.astype(np.int32), row.astype(np.int32)
    return out


def model_performance(gt_classes, classes, gt_boxes, boxes):
    """(misclassification rate, mIoU, RMSE) of model_performance.txt (validate_model.py:706-735).  RMSE = sqrt(mean((pred -
    gt)^2 over the ELEMENTS where gt != 0)) (utils_box.py:92-103); the reference reduces in TensorFlow float32 in an order
    that is not pinned, here it is a float64 mean."""
    gt_classes, classes = np.asarray(gt_classes), np.asarray(classes)
    gt_boxes, boxes = np.asarray(gt_boxes, np.float32), np.asarray(boxes, np.float32)
    mis = len(np.where(gt_classes != classes)[0]) / len(gt_classes)
    miou = float(np.mean(calc_iou_np(gt_boxes, boxes)))
    sq = np.square(boxes.astype(np.float64) - gt_boxes.astype(np.float64))[gt_boxes != 0.0]
    return mis, miou, float(np.sqrt(np.mean(sq)))


class RefDriver:
    """The host flow a user of `serve()` alone has to write: a stand-in for `ServingDriver` in `writers.validate_to_file` /
    `calibration.gather_detections` whose `assign_ground_truth` is this file applied to the detections `serve_fn(batch)`
    returned (and `probs_fn(n)` -> (probab, entropy) when the configuration has logits)."""

    def __init__(self, params, serve_fn, probs_fn=None):
        self.params, self._serve, self._probs = params, serve_fn, probs_fn
        self.M = int(params["nms_configs"]["max_output_size"])

    def serve_stream(self, batches, post_mode=None, while_resident=None):
        for b in batches:
            self._det = self._serve(b)
            yield self._det if while_resident is None else while_resident(self._det)

    def assign_ground_truth(self, gt_boxes, gt_classes, method=None, keep="validate"):
        method = self.params.get("assign_gt_box") if method is None else method
        gb, gc = np.asarray(gt_boxes, np.float32), np.asarray(gt_classes, np.float32)
        idx, iou, count = assign(method, gb, gc, self._det[0], keep)
        probab = entropy = None
        if self.params["enable_softmax"]:
            probab, entropy = self._probs(self._det[0].shape[0])
        out = dict(det_index=idx, iou=iou, count=count)
        out.update(gather(self.params, self._det, idx, gb, gc, probab, entropy, keep))
        return out
