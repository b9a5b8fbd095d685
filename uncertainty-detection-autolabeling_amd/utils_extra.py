"""MC-dropout helpers of the reference's `utils_extra` on the HIP path (src/utils_extra.py:119-244).

  mc_infer(driver, image, T=10)        serving-level twin: T serve() calls stacked            (:119-139)
  mc_eval(mc_model, images, config)    model-level twin used by eval.py:108-112 / train_lib   (:142-198)
  stack_mcpred / get_mcuncert          stacking and mean / population std over the sample axis (:201-244)
  gt_box_assigner / assign_gt_boxes    the detection that belongs to a ground-truth box, on the device       (:44-64)

`mc_eval` on an `efficientdet_keras.EfficientDetNet` of this package runs the T stochastic passes as ONE
launch sequence with the sample axis explicit (weights read once, everything upstream of the first dropout
site computed once per image) instead of T model calls; the result has the reference's structure - per
level [T,N,h,w,ch] for a head whose (or the global) rate is non-zero, else the deterministic output.
"""
import numpy as np


def mc_infer(driver, image, T=10):
    """T calls of `driver.serve(image)`, each output stacked on a new axis 0 (src/utils_extra.py:119-139)."""
    runs = [driver.serve(image) for _ in range(T)]
    return [np.stack([np.asarray(r[i]) for r in runs], axis=0) for i in range(len(runs[0]))]


def stack_mcpred(output):
    """[[level-0 samples], ..., [level-4 samples]] -> five arrays stacked on axis 0 (:201-217)."""
    return [np.stack([np.asarray(x) for x in lvl], axis=0) for lvl in output]


def get_mcuncert(output):
    """(mean, population std) over axis 0 of each of the five stacked arrays (:220-244); sequential float32 sums,
    the order the HIP aggregate kernel and the oracle use."""
    means, stds = [], []
    for x in output:
        x = np.asarray(x, dtype=np.float32)
        acc = x[0].copy()
        for t in range(1, x.shape[0]):
            acc = acc + x[t]
        m = acc / np.float32(x.shape[0])
        v = np.zeros_like(m)
        for t in range(x.shape[0]):
            d = x[t] - m
            v = v + d * d
        means.append(m)
        stds.append(np.sqrt(v / np.float32(x.shape[0])))
    return means, stds


def mc_eval(mc_model, images, config):
    """[cls_outputs, box_outputs] with the MC samples stacked (src/utils_extra.py:142-198)."""
    if hasattr(mc_model, "mc_forward"):           # this package's EfficientDetNet: one run, explicit sample axis
        return mc_model.mc_forward(images)
    # any other callable with the reference's model signature: the reference's loop
    stack_c = bool(config.mc_classheadrate or config.mc_dropoutrate)
    stack_b = bool(config.mc_boxheadrate or config.mc_dropoutrate)
    cls_runs, box_runs = [], []
    cls = box = None
    for _ in range(config.mc_dropoutsamp):
        cls, box = mc_model(images, training=False)
        cls_runs.append(cls)
        box_runs.append(box)
    cls_concat = stack_mcpred([[r[l] for r in cls_runs] for l in range(len(cls))]) if stack_c else cls
    box_concat = stack_mcpred([[r[l] for r in box_runs] for l in range(len(box))]) if stack_b else box
    return [cls_concat, box_concat]


# ------------------------------------------------------------------ ground-truth assignment (:44-64)
KEEP_RULES = ("validate", "calibrate")


def assign_method_code(method):
    """model_params["assign_gt_box"] -> the C enum: "IoU" 0, "MSE" 1, anything else 2 (the reference's else branch: the
    GT row's own rank)."""
    from . import capi
    return {"IoU": capi.ASSIGN_IOU, "MSE": capi.ASSIGN_MSE}.get(method, capi.ASSIGN_RANK)


def keep_code(keep):
    from . import capi
    if keep not in KEEP_RULES:
        raise ValueError("keep must be one of %s, got %r" % (KEEP_RULES, keep))
    return capi.ASSIGN_KEEP_CALIBRATE if keep == "calibrate" else capi.ASSIGN_KEEP_VALIDATE


def check_ground_truth(gt_boxes, gt_classes):
    """(gt_boxes [n, G, 4], gt_classes [n, G]) as contiguous float32 - the dtype the reference's eval dataloader hands over
    (inspector.py:147-160), padded with -1 rows.  ValueError on any other shape and on non-finite values."""
    gb = np.ascontiguousarray(gt_boxes, dtype=np.float32)
    gc = np.ascontiguousarray(gt_classes, dtype=np.float32)
    if gb.ndim != 3 or gb.shape[-1] != 4:
        raise ValueError("gt_boxes must be [n, G, 4], got %s" % (gb.shape,))
    if gc.shape != gb.shape[:2]:
        raise ValueError("gt_classes must be [n, G] = %s, got %s" % (gb.shape[:2], gc.shape))
    if gb.shape[0] < 1:
        raise ValueError("ground truth of zero images")
    if not (np.isfinite(gb).all() and np.isfinite(gc).all()):
        raise ValueError("ground-truth boxes and classes must be finite")
    return gb, gc


def check_rank_rows(method, gc, M, keep):
    """The rank branch pairs GT row i with detection i: a kept row i >= M has none (the reference would index past the
    detections there)."""
    if assign_method_code(method) != 2 or keep == "calibrate":      # calibrate keeps rows < min(G, M) only
        return
    rows = np.nonzero(gc > 0)[1]
    if rows.size and rows.max() >= M:
        raise ValueError("assign_gt_box=%r pairs ground-truth row i with detection i, but kept row %d is beyond the %d "
                         "detections" % (method, int(rows.max()), M))


def assign_gt_boxes(method, gt_boxes, gt_classes, boxes, keep="validate", device=0):
    """`gt_box_assigner` for whole batches, on the device (`uda_assign_gt_np`, the kernel `ServingDriver.assign_ground_truth`
    runs): gt_boxes [n, G, 4], gt_classes [n, G] (-1 rows: padding), boxes [n, M, >= 4] detections of one's own ->
    (det_index [n, G] int32, -1 = row not kept; iou [n, G] float64 of each GT box with its detection; count [n] int32).
    keep="validate": rows with class > 0 (validate_model.py:314); "calibrate": rows < min(G, M) with class >= 0
    (calibrate_model.py:133-135).  Ties go to the lowest rank, as np.argmax / np.argmin do."""
    from . import capi
    gb, gc = check_ground_truth(gt_boxes, gt_classes)
    b = np.asarray(boxes, dtype=np.float32)
    if b.ndim != 3 or b.shape[0] != gb.shape[0] or b.shape[-1] < 4:
        raise ValueError("boxes must be [n = %d, M, >= 4], got %s" % (gb.shape[0], b.shape))
    b = np.ascontiguousarray(b[..., :4])
    n, G, M = gb.shape[0], gb.shape[1], b.shape[1]
    kc = keep_code(keep)
    check_rank_rows(method, gc, M, keep)
    if M == 0 and keep == "validate" and (gc > 0).any():     # (calibrate keeps rows < min(G, M) only)
        raise ValueError("a kept ground-truth row and no detection to match it with (the reference fails in np.argmax)")
    if not np.isfinite(b).all():
        raise ValueError("detection boxes must be finite")
    idx = np.full((n, G), -1, np.int32)
    iou = np.zeros((n, G), np.float64)
    count = np.zeros((n,), np.int32)
    lib = capi.load()
    rc = lib.uda_assign_gt_np(int(device), b.ctypes.data, gb.ctypes.data, gc.ctypes.data, n, M, G, assign_method_code(method),
                              kc, idx.ctypes.data, iou.ctypes.data, count.ctypes.data)
    capi.check(lib, None, rc, "uda_assign_gt_np")
    return idx, iou, count


def gt_box_assigner(sorting_method, gt_box, boxes, i, device=0):
    """The reference's call shape (:44-64): gt_box [G, 4], boxes [M, 4] of one image, GT row i -> the matched rank."""
    gt_box = np.asarray(gt_box, dtype=np.float32)
    if assign_method_code(sorting_method) == 2:
        return int(i)
    idx, _, _ = assign_gt_boxes(sorting_method, gt_box[None, i:i + 1], np.ones((1, 1), np.float32), np.asarray(boxes)[None],
                                device=device)
    return int(idx[0, 0])
