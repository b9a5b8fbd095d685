"""The on-disk records every downstream experiment parses.

  prediction_data.txt   one python-dict literal per detection above the score threshold, as `Infer.iterate_infer`
                        writes it (reference src/infer_model.py:836-960, `add_array_dict` utils_extra.py:67-81)
  validate_results.txt  one dict per detection matched to a ground-truth box, as `Validate.launch_val` writes it
                        (src/validate_model.py:524-681), plus the runtime summary of validationstep_runtime.txt
                        (:685-704), average_score.txt (:683-684) and model_performance.txt (:706-735):
                        `validate_to_file` is that whole loop
  corrected ground truth the KITTI label files and the BDD100K json of `AdvancedLabels.corrected_gt` (src/ssl_utils/glc.py:231-406)
                        for the verdicts of a `label_correction.LabelCheck`: `write_kitti_corrected_gt`, `write_bdd_corrected_gt`
  corrected pseudo labels the KITTI label files and the BDD100K json of `ThreeDproblem.corrected_pseudo` (src/ssl_utils/3d.py:80-255)
                        for a `pseudo_audit.PseudoCorrection`: `write_kitti_corrected_pseudo`, `write_bdd_corrected_pseudo`
  epistemic vs aleatoric  the two text files of `EpistemicVSAleatoric.save_highlow` (src/uncertainty_ep_vs_al.py:393-449) for an
                        `epal.EpalComparison`: `write_epal_highlow`

Both are read back with `ast.literal_eval(line.replace("inf", "2e308"))` (active_learning_loop.py:532,
SSL_stac.py:345, uncertainty_analysis.py).  The reference prints numpy-1 float32 scalars, whose repr is the shortest
decimal that round-trips in float32 ('0.1234', not '0.12340000271797180'); the values are written here as the python
float with that shortest repr, so a line is text-identical to the reference's for the same numbers.  Key order follows
the reference statement by statement (it differs between the two files: albox before mcbox in prediction_data,
mcbox before albox in validate_results).
"""
import numpy as np

CLASS_CALIB_KEYS_INFER = ("ts_all", "ts_percls", "iso_all", "iso_percls")          # infer_model.py:868-893, 903-915
CLASS_CALIB_KEYS_VAL = ("iso_all", "ts_all", "ts_percls", "iso_percls")            # validate_model.py:547-590, 597-618
BOX_CALIB_KEYS_INFER = ("iso_all", "ts_all", "ts_percoo", "iso_percoo", "iso_perclscoo", "rel_iso_perclscoo")
BOX_CALIB_KEYS_VAL = BOX_CALIB_KEYS_INFER                                          # validate_model.py:625-655


def _f32(v):
    """python float that prints like numpy 1's repr of the float32 value v."""
    return float(str(np.float32(v)))


def _f32_list(a):
    return [_f32(v) for v in np.ravel(np.asarray(a))]


def add_array_dict(data_dict, source_array, target_key, select_index):
    """utils_extra.add_array_dict (:67-81): rounded (4 decimals), NaN-free copy of row `select_index` under `target_key`."""
    source_array = np.asarray(source_array)
    if source_array.size > 0:
        vals = np.nan_to_num(np.around(source_array[select_index].astype("float32"), 4))
        data_dict[target_key] = _f32_list(vals) if np.size(source_array[select_index]) > 1 else _f32(vals)
    return data_dict


def prediction_records(unpacked, image_names, min_score, calibrated=None, calibrate_classification=True,
                       calibrate_regression=True, consistency=None):
    """Records of `ServingDriver.serve_unpacked` output for a batch, in the reference's key order
    (infer_model.py:836-960).

    calibrated: optional dict name -> [N, M, ...] arrays written behind the uncalibrated column they refine:
    "<method>_probab" / "<method>_entropy" / "<method>_mcclass" (`ClassCalibrator`), "<method>_albox" /
    "<method>_mcbox" (`BoxCalibrator`); a missing name is skipped like the reference's empty array.
    consistency: optional (cons_iou [N, M], cons_cls [N, M]) of `ServingDriver.serve_consistency`, written right after
    "class" as the reference does under consistency_ssl (:842-844): a float64 and a python bool."""
    recs = []
    cal = calibrated or {}
    boxes, scores, classes = unpacked["boxes"], unpacked["scores"], unpacked["classes"]

    def add_cal(d, names, suffix, i, sel):
        for m in names:
            key = "%s_%s" % (m, suffix)
            if key in cal:
                add_array_dict(d, np.asarray(cal[key])[i], key, sel)

    for i, name in enumerate(image_names):
        # the reference mutates ONE dict per image: a key written for an earlier detection stays in the later lines
        d = {"image_name": name + ".jpg", "score_thresh": float(min_score), "top_5scores": _f32_list(scores[i][:5])}
        for sel in np.where(scores[i] > min_score)[0]:
            d["det_score"] = _f32(scores[i][sel])
            d["bbox"] = _f32_list(boxes[i][sel])
            d["class"] = _f32(classes[i][sel])
            if consistency is not None:
                d["cons_iou"] = float(consistency[0][i][sel])
                d["cons_cls"] = bool(consistency[1][i][sel])
            if unpacked.get("logits") is not None:
                add_array_dict(d, unpacked["logits"][i], "logits", sel)
                add_array_dict(d, unpacked["entropy"][i], "entropy", sel)
                d["probab"] = _f32_list(unpacked["probab"][i][sel])
                if calibrate_classification:
                    add_cal(d, CLASS_CALIB_KEYS_INFER, "probab", i, sel)
                    add_cal(d, CLASS_CALIB_KEYS_INFER, "entropy", i, sel)
            if unpacked.get("mcclass") is not None:
                add_array_dict(d, unpacked["mcclass"][i], "uncalib_mcclass", sel)
                if calibrate_classification:
                    add_cal(d, CLASS_CALIB_KEYS_INFER, "mcclass", i, sel)
            if unpacked.get("albox") is not None:
                add_array_dict(d, unpacked["albox"][i], "uncalib_albox", sel)
                if calibrate_regression:
                    add_cal(d, BOX_CALIB_KEYS_INFER, "albox", i, sel)
            if unpacked.get("mcbox") is not None:
                add_array_dict(d, unpacked["mcbox"][i], "uncalib_mcbox", sel)
                if calibrate_regression:
                    add_cal(d, BOX_CALIB_KEYS_INFER, "mcbox", i, sel)
            recs.append(dict(d))
    return recs


def write_prediction_data(path, records):
    """Append one `str(dict)` line per record (infer_model.py:956-960)."""
    with open(path, "a") as f:
        for r in records:
            f.write(str(r) + "\n")


def predict_to_file(driver, batches, names, path, min_score, box_calibrator=None, class_calibrator=None,
                    box_methods=(), class_methods=()):
    """The inference flow of `Infer.iterate_infer` (infer_model.py:554-960) as ONE loop over batches of images (arrays, or
    lists of images of different raw sizes): serve (feed of the next batch hidden under this one) -> unpack + softmax /
    entropy (device) -> calibrated box / class uncertainties (device, `calibration.BoxCalibrator` / `ClassCalibrator`)
    -> `prediction_data.txt` lines appended to `path`.  `names`: one list of image names per batch.  Returns the number
    of records written.  With `driver.params["consistency_ssl"]` every batch goes through `serve_consistency` (one device
    run of the images and their flip / blur / noise variants, not pipelined) and the records carry cons_iou / cons_cls
    (infer_model.py:768-848)."""
    from . import postprocess as pp
    names = list(names)
    state = {"i": 0, "written": 0}

    def per_batch(det, consistency=None):
        n = det[0].shape[0]
        rows = 4 * n if consistency is not None else n       # images the handle holds: the variants follow the originals
        probs = ent = None
        if driver.params["enable_softmax"]:
            probs, ent = (a[:n] for a in driver.class_probs(rows))
        un = pp.unpack_detections(driver.params, det, probs, ent)
        cal = {}
        if box_calibrator is not None:
            for m in box_methods:
                for which in ("albox", "mcbox"):
                    if un.get(which) is not None:
                        cal["%s_%s" % (m, which)] = box_calibrator.calibrate_boxuncert(rows, which, m)[:n]
        if class_calibrator is not None and un.get("logits") is not None:
            for m in class_methods:
                r = class_calibrator.perform_class_calib(rows, m)
                cal[m + "_entropy"], cal[m + "_probab"] = r[0][:n], r[1][:n]
                if len(r) > 2:
                    cal[m + "_mcclass"] = r[2][:n]
        recs = prediction_records(un, names[state["i"]], min_score, cal, consistency=consistency)
        write_prediction_data(path, recs)
        state["i"] += 1
        state["written"] += len(recs)
        return len(recs)

    if driver.params.get("consistency_ssl"):
        for batch in batches:
            det, cons_iou, cons_cls = driver.serve_consistency(batch)
            per_batch(det, (cons_iou, cons_cls))
        return state["written"]
    for _ in driver.serve_stream(batches, while_resident=per_batch):
        pass
    return state["written"]


def validate_records(filtered, params, calibrated=None):
    """Records of `validate_results.txt` (validate_model.py:524-681) from the per-detection arrays the validation
    harness keeps after ground-truth assignment (CPU numpy analysis outside the hot path).

    filtered: dict with `names` [K] str, `scores` [K], `boxes` [K,4], `gt_boxes` [K,4], `occlusions` [K],
    `truncations` [K], `classes` [K], `gt_classes` [K] and, as the configuration produces them, `logits` [K,C],
    `probab` [K,C], `entropy` [K], `mcclass` [K,C], `mcbox` [K,4], `albox` [K,4].
    calibrated: optional dict "<method>_<probab|entropy|mcclass|mcbox|albox>" -> [K, ...]."""
    cal = calibrated or {}
    recs = []
    K = len(filtered["boxes"])

    def add_cal(d, names, suffix, i):
        for m in names:
            key = "%s_%s" % (m, suffix)
            if key in cal:
                add_array_dict(d, np.asarray(cal[key]), key, i)

    for i in range(K):
        d = {"image_name": filtered["names"][i], "score": _f32(filtered["scores"][i]), "bbox": _f32_list(filtered["boxes"][i]),
             "gt_bbox": _f32_list(filtered["gt_boxes"][i]), "gt_occl": _plain(filtered["occlusions"][i]),
             "gt_trunc": _plain(filtered["truncations"][i]), "class": _plain(filtered["classes"][i]),
             "gt_class": _plain(filtered["gt_classes"][i])}
        if params["enable_softmax"]:
            d["logits"] = _f32_list(filtered["logits"][i])
            d["probab"] = _f32_list(filtered["probab"][i])
            d["entropy"] = _f32(filtered["entropy"][i])
            if params.get("calibrate_classification"):
                add_cal(d, CLASS_CALIB_KEYS_VAL, "probab", i)
                add_cal(d, CLASS_CALIB_KEYS_VAL, "entropy", i)
        if params.get("mc_classheadrate") or params.get("mc_dropoutrate"):
            d["uncalib_mcclass"] = _f32_list(filtered["mcclass"][i])
            if params.get("calibrate_classification"):
                add_cal(d, CLASS_CALIB_KEYS_VAL, "mcclass", i)
        if params.get("mc_boxheadrate") or params.get("mc_dropoutrate"):
            d["uncalib_mcbox"] = _f32_list(filtered["mcbox"][i])
            if params.get("calibrate_regression"):
                add_cal(d, BOX_CALIB_KEYS_VAL, "mcbox", i)
        if params.get("loss_attenuation"):
            d["uncalib_albox"] = _f32_list(filtered["albox"][i])
            if params.get("calibrate_regression"):
                add_cal(d, BOX_CALIB_KEYS_VAL, "albox", i)
        recs.append(d)
    return recs


def _plain(v):
    """ints stay ints, float32 scalars print like numpy 1 (ground-truth fields come from the label files)."""
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return _f32(v) if isinstance(v, np.float32) else float(v)
    return v


def write_validate_results(path, records):
    """One `str(dict)` line per record, file rewritten (validate_model.py:526, :681)."""
    with open(path, "w") as f:
        for r in records:
            f.write(str(r) + "\n")


def write_epal_highlow(out_dir, comparison):
    """`EpistemicVSAleatoric.save_highlow` (uncertainty_ep_vs_al.py:393-449) without the crop montages: under
    out_dir/compare_epal/mcdropout (or .../entropy, :479, :486) the files hal_lep_<uncert>_iou_<thr>.txt and lal_hep_..., one
    `str(record)` line per detection of the "high AL / low EP" and of the "low AL / high EP" corner, files rewritten.  Returns the
    two paths."""
    import os
    folder = os.path.join(out_dir, comparison.subdir)
    os.makedirs(folder, exist_ok=True)
    paths = []
    for stem, recs in zip(("hal_lep", "lal_hep"), comparison.highlow_records()):
        paths.append(os.path.join(folder, "%s_%s_iou_%s.txt" % (stem, comparison.uncert, str(comparison.iou_thr))))
        with open(paths[-1], "w") as f:
            for r in recs:
                f.write(str(r) + "\n")
    return tuple(paths)


def summarize_runtimes(seconds):
    """The three lines `Validate.launch_val` leaves in validationstep_runtime.txt (validate_model.py:685-704): per-image
    serve() wall clock, calls of 1 s or more dropped, then outliers above q3 + 50 IQR dropped; mean / std / median in ms."""
    t = np.asarray(seconds, np.float32)
    t = t[t < 1]
    q3 = np.percentile(t, 75)
    iqr = np.percentile(t, 75) - np.percentile(t, 25)
    kept = [x for x in t if x <= q3 + 50 * iqr]
    return ["Mean time in ms: {:.3f}\n".format(np.mean(kept) * 1000), "STD time in ms: {:.3f}\n".format(np.std(kept) * 1000),
            "Median time in ms: {:.3f}\n".format(np.median(kept) * 1000)]


def model_performance(filtered):
    """The three lines of model_performance.txt (validate_model.py:706-735) from the matched rows: share of rows whose
    class differs from the ground truth's, mean IoU (`filtered["iou"]`: calc_iou_np of each GT box with its detection), and
    RMSE over the box ELEMENTS where the ground truth is not 0 (utils_box.py:92-103).  The reference takes the RMSE as a
    TensorFlow float32 reduce_mean whose summation order is not pinned; here it is a float64 mean."""
    gt_cls, cls = np.asarray(filtered["gt_classes"]), np.asarray(filtered["classes"])
    gt, b = np.asarray(filtered["gt_boxes"], np.float32), np.asarray(filtered["boxes"], np.float32)
    mis = len(np.where(gt_cls != cls)[0]) / len(gt_cls)
    sq = np.square(b.astype(np.float64) - gt.astype(np.float64))[gt != 0.0]
    return ["Misclassification rate: {}\n".format(mis), "mIoU: {}\n".format(float(np.mean(filtered["iou"]))),
            "RMSE: {}\n".format(float(np.sqrt(np.mean(sq))))]


def validate_to_file(driver, batches, gts, names, out_dir, box_calibrator=None, class_calibrator=None, occlusions=None,
                     truncations=None, class_report=None, uncert_report=False):
    """The loop of `Validate.launch_val` (validate_model.py:472-735) without its `infer_augment` branches, over batches
    of images: serve (feed of the next batch hidden under this one, as in `predict_to_file`) -> ground-truth assignment on
    the resident detections (`ServingDriver.assign_ground_truth`, method model_params["assign_gt_box"]) -> calibrated
    columns of every method the calibrators hold a model for, gathered on the host with `det_index` -> files in `out_dir`:

      validate_results.txt          `validate_records` / `write_validate_results`
      average_score.txt             mean matched score (:683-684; the reference accumulates the scores in float64)
      validationstep_runtime.txt    `summarize_runtimes` of the per-image serve time (batch time / images, the assignment
                                    and the writing excluded, as the reference times serve() alone, :154-158)
      model_performance.txt         only without box uncertainty (no MC box dropout, no loss attenuation), as the reference
                                    (:706-735); `model_performance`.  With `uncert_report` and box uncertainty: the
                                    lines `ValidUncertPlot.__init__` appends instead (:736-794, utils_extra.py:417-445),
                                    aleatoric first, of the second kind the ECE line alone (the file exists by then, as
                                    it does for both kinds when a previous run left one) - `uncertainty_report`, one
                                    device call over the matched rows; the report is returned as filtered["uncert_report"]

    gts: per batch (gt_boxes [n, G, 4], gt_classes [n, G]); names: per batch the n image file names; occlusions /
    truncations: per batch [n, G] label fields (None: written as 0).  Returns the matched-row arrays (`filtered`).

    class_report: None (default: nothing changes), or the models dict a `ClassCalibrator` takes ({}: the uncalibrated table
    alone) - then filtered["class_report"] is the classification calibration report of ALL matched rows (`class_report.
    from_filtered(filtered, models, split=0, one_based=True)`: reliability bins, ECE, MCE, Brier, NLL, SCE of every table from
    one device call; the models were fitted elsewhere, so no row is held back).  No file is written for it."""
    import os
    import time
    p = driver.params
    gts, names = list(gts), list(names)
    keys = ("scores", "boxes", "classes", "logits", "probab", "entropy", "mcclass", "mcbox", "albox", "gt_boxes", "gt_classes")
    acc = {k: [] for k in keys + ("names", "occlusions", "truncations", "iou")}
    cal_acc = {}
    state = {"i": 0, "inside": 0.0}
    seconds = []

    def per_batch(det):
        t0 = time.time()
        b = state["i"]
        n = det[0].shape[0]
        asg = driver.assign_ground_truth(gts[b][0], gts[b][1], keep="validate")
        im, row, k = asg["image"], asg["gt_row"], asg["det_index"][asg["image"], asg["gt_row"]]
        for key in keys:
            if asg[key] is not None:
                acc[key].append(asg[key])
        acc["iou"].append(asg["iou"][im, row])
        acc["names"] += [names[b][i] for i in im]
        for key, src in (("occlusions", occlusions), ("truncations", truncations)):
            acc[key].append(np.zeros(len(im), np.int64) if src is None else np.asarray(src[b])[im, row])
        if box_calibrator is not None and p.get("calibrate_regression"):
            for which in ("albox", "mcbox"):
                if asg[which] is not None:
                    for m in box_calibrator.models:
                        cal_acc.setdefault("%s_%s" % (m, which), []).append(box_calibrator.calibrate_boxuncert(n, which, m)[im, k])
        if class_calibrator is not None and p.get("calibrate_classification") and asg["logits"] is not None:
            for m in class_calibrator.models:
                r = class_calibrator.perform_class_calib(n, m)
                cal_acc.setdefault(m + "_entropy", []).append(r[0][im, k])
                cal_acc.setdefault(m + "_probab", []).append(r[1][im, k])
                if len(r) > 2:
                    cal_acc.setdefault(m + "_mcclass", []).append(r[2][im, k])
        state["i"] += 1
        state["inside"] = time.time() - t0
        return n

    it = driver.serve_stream(batches, while_resident=per_batch)
    while True:
        t0 = time.time()
        n = next(it, None)
        if n is None:
            break
        seconds += [(time.time() - t0 - state["inside"]) / n] * n

    filtered = {k: (np.concatenate(v) if v else None) for k, v in acc.items() if k != "names"}
    filtered["names"] = acc["names"]
    cal = {k: np.concatenate(v) for k, v in cal_acc.items()}
    os.makedirs(out_dir, exist_ok=True)
    if filtered["boxes"] is None:
        raise ValueError("validate_to_file: no batches")
    write_validate_results(os.path.join(out_dir, "validate_results.txt"), validate_records(filtered, p, cal))
    with open(os.path.join(out_dir, "average_score.txt"), "w") as f:
        f.write(str(np.mean(filtered["scores"].astype(np.float64))))
    with open(os.path.join(out_dir, "validationstep_runtime.txt"), "w") as f:
        f.writelines(summarize_runtimes(seconds))
    if not (p.get("mc_boxheadrate") or p.get("mc_dropoutrate")) and not p.get("loss_attenuation"):
        with open(os.path.join(out_dir, "model_performance.txt"), "w") as f:
            f.writelines(model_performance(filtered))
    filtered["calibrated"] = cal
    if uncert_report and ((p.get("mc_boxheadrate") or p.get("mc_dropoutrate")) or p.get("loss_attenuation")):
        from . import uncertainty_report
        rep = uncertainty_report.from_filtered(filtered, calibrated=True, device=getattr(driver, "device", 0))
        path = os.path.join(out_dir, "model_performance.txt")
        for which, has in (("aleatoric", p.get("loss_attenuation")), ("mcdropout", p.get("mc_boxheadrate") or p.get("mc_dropoutrate"))):
            if has:
                lines = uncertainty_report.model_performance_lines(rep, which, p["uncert_adjust_method"], exists=os.path.exists(path))
                with open(path, "a") as f:
                    f.writelines(lines)
        filtered["uncert_report"] = rep
    if class_report is not None:
        from . import class_report as class_report_mod
        filtered["class_report"] = class_report_mod.from_filtered(filtered, class_report, split=0, one_based=True,
                                                                  device=getattr(driver, "device", 0))
    return filtered


# ---------------------------------------------------------------------------------- corrected ground truth (label correction)
def _verdicts(check, wrong_gt, corrected_gt_boxes, missing_gt_boxes, pred_boxes, pred_classes):
    """The lists `AdvancedLabels.corrected_gt` takes, each from `check` (a `label_correction.LabelCheck`) unless given."""
    if check is not None:
        wrong_gt = check.wrong_gt if wrong_gt is None else wrong_gt
        corrected_gt_boxes = check.corrected_gt_boxes if corrected_gt_boxes is None else corrected_gt_boxes
        missing_gt_boxes = check.extra_correct_dets if missing_gt_boxes is None else missing_gt_boxes
        pred_boxes = check.pred_boxes if pred_boxes is None else pred_boxes
        pred_classes = check.pred_classes if pred_classes is None else pred_classes
    return wrong_gt, corrected_gt_boxes, missing_gt_boxes, pred_boxes, pred_classes


def _need(flag, what, **lists):
    for name, v in lists.items():
        if flag and v is None:
            raise ValueError("%s needs %s (or a LabelCheck)" % (what, name))


def write_kitti_corrected_gt(gt_labels_dir, out_dir, file_names, used_classes, check=None, remove_mistakes=False, wrong_gt=None,
                             correct_boxes=False, corrected_gt_boxes=None, add_missingboxes=False, missing_gt_boxes=None,
                             pred_boxes=None, pred_classes=None):
    """The KITTI label files of `AdvancedLabels.corrected_gt` (glc.py:231-306): for image i the lines of
    gt_labels_dir/file_names[i] whose class is one of `used_classes`, in order, row j counting over those lines -
    remove_mistakes drops the rows in wrong_gt[i]; correct_boxes rewrites fields 4-7 of the rows that stay with
    corrected_gt_boxes[i][j] (x1 y1 x2 y2, `str` of the python float: an untouched box loses its file's formatting, as in the
    reference); add_missingboxes appends one 15-field line per detection b with missing_gt_boxes[i][b], class
    used_classes[int(pred_classes[i][b]) - 1], box pred_boxes[i][b].  A float32 coordinate must be given as the number the
    reference reads back from its file (the shortest decimal; `LabelCheck` does that).  The lists come from `check` unless
    given.  Writes out_dir/file_names[i]; returns the number of lines written.  (TFRecords are not written.)"""
    import os
    wrong_gt, corrected_gt_boxes, missing_gt_boxes, pred_boxes, pred_classes = _verdicts(
        check, wrong_gt, corrected_gt_boxes, missing_gt_boxes, pred_boxes, pred_classes)
    _need(remove_mistakes, "remove_mistakes", wrong_gt=wrong_gt)
    _need(correct_boxes, "correct_boxes", corrected_gt_boxes=corrected_gt_boxes)
    _need(add_missingboxes, "add_missingboxes", missing_gt_boxes=missing_gt_boxes, pred_boxes=pred_boxes, pred_classes=pred_classes)
    os.makedirs(out_dir, exist_ok=True)
    written = 0
    for i, fname in enumerate(file_names):
        out_lines = []
        with open(os.path.join(gt_labels_dir, fname), "r") as f:
            j = 0
            for line in f.readlines():
                parts = line.strip().split(" ")
                if len(parts) > 0 and parts[0] in used_classes:
                    keep = not (remove_mistakes and j in wrong_gt[i])
                    if correct_boxes and keep:
                        box = corrected_gt_boxes[i][j]
                        parts[4], parts[5], parts[6], parts[7] = str(box[1]), str(box[0]), str(box[3]), str(box[2])
                    if keep:
                        out_lines.append(parts)
                    j += 1
        if add_missingboxes:
            for b in range(len(pred_boxes[i])):
                if missing_gt_boxes[i][b]:
                    box = pred_boxes[i][b]
                    out_lines.append([used_classes[int(pred_classes[i][b]) - 1], "-1", "-1", "-10", str(box[1]), str(box[0]),
                                      str(box[3]), str(box[2]), "-1", "-1", "-1", "-1000", "-1000", "-1000", "-10"])
        with open(os.path.join(out_dir, fname), "w") as f:
            f.writelines([" ".join(item) + "\n" for item in out_lines])
        written += len(out_lines)
    return written


def write_bdd_corrected_gt(bdd_data, out_dir, image_names, used_classes, check=None, remove_mistakes=False, wrong_gt=None,
                           correct_boxes=False, corrected_gt_boxes=None, add_missingboxes=False, missing_gt_boxes=None,
                           pred_boxes=None, pred_classes=None):
    """The BDD100K json of `AdvancedLabels.corrected_gt` (glc.py:327-406): bdd_data is the loaded label json (a list of items) or
    its path; the items that carry a "labels" list and whose name is in `image_names` are written, in the JSON's order, with
    the objects whose category is one of `used_classes` (row j counting over those) - the three modes as in
    `write_kitti_corrected_gt`; an added object gets id str(j + b), the reference's attributes and the detection's box.  The
    reference applies verdict i to the i-th written item: the items must therefore come in the order of `image_names`, and an
    order that would pair an item with another image's verdicts is refused (the reference mislabels it silently).  The input
    is not modified.  Writes out_dir/bdd100k_labels_images_train.json (json.dump, indent=4); returns the number of objects."""
    import copy
    import json
    import os
    wrong_gt, corrected_gt_boxes, missing_gt_boxes, pred_boxes, pred_classes = _verdicts(
        check, wrong_gt, corrected_gt_boxes, missing_gt_boxes, pred_boxes, pred_classes)
    _need(remove_mistakes, "remove_mistakes", wrong_gt=wrong_gt)
    _need(correct_boxes, "correct_boxes", corrected_gt_boxes=corrected_gt_boxes)
    _need(add_missingboxes, "add_missingboxes", missing_gt_boxes=missing_gt_boxes, pred_boxes=pred_boxes, pred_classes=pred_classes)
    if isinstance(bdd_data, str):
        with open(bdd_data, "r") as f:
            bdd_data = json.load(f)
    image_names = [str(nm) for nm in image_names]
    wanted = set(image_names)
    filtered_data, written, i = [], 0, 0
    for item in bdd_data:
        if "labels" in item and isinstance(item["labels"], list) and item["name"] in wanted:
            if i >= len(image_names) or image_names[i] != item["name"]:
                raise ValueError("write_bdd_corrected_gt: item %d of the json that is written is %r, the verdicts at that place belong "
                                 "to %r: order image_names like the json" % (i, item["name"], image_names[min(i, len(image_names) - 1)]))
            filtered_item = dict(item)
            objs, j = [], 0
            for obj in item["labels"]:
                obj = copy.deepcopy(obj)
                if obj["category"] in used_classes:
                    keep = not (remove_mistakes and j in wrong_gt[i])
                    if correct_boxes and keep:
                        box = corrected_gt_boxes[i][j]
                        obj["box2d"]["x1"], obj["box2d"]["y1"], obj["box2d"]["x2"], obj["box2d"]["y2"] = box[1], box[0], box[3], box[2]
                    if keep:
                        objs.append(obj)
                    j += 1
            if add_missingboxes:
                for b in range(len(pred_boxes[i])):
                    if missing_gt_boxes[i][b]:
                        box = pred_boxes[i][b]
                        objs.append({"id": str(j + b), "attributes": {"occluded": False, "truncated": False, "trafficLightColor": "G"},
                                     "category": used_classes[int(pred_classes[i][b] - 1)],
                                     "box2d": {"x1": box[1], "y1": box[0], "x2": box[3], "y2": box[2]}})
            filtered_item["labels"] = objs
            filtered_data.append(filtered_item)
            written += len(objs)
            i += 1
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bdd100k_labels_images_train.json"), "w") as f:
        json.dump(filtered_data, f, indent=4)
    return written


# ---------------------------------------------------------------------------------- corrected pseudo labels (pseudo-label audit)
def _audit_sizes(who, name, n_pred, n_gt, audit, i):
    if n_pred != audit.n_pred_perim[i] or n_gt != audit.n_gts_perim[i]:
        raise ValueError("%s: image %r has %d pseudo labels and %d ground-truth rows of the used classes, the audit saw %d and %d"
                         % (who, name, n_pred, n_gt, audit.n_pred_perim[i], audit.n_gts_perim[i]))


def write_kitti_corrected_pseudo(det_folder, gt_labels_folder, out_dir, used_classes, audit, correction):
    """The KITTI files of `ThreeDproblem.corrected_pseudo` (3d.py:115-164) for a `pseudo_audit.PseudoAudit` whose names are the
    file names and a `PseudoCorrection` of it: per image the lines of det_folder/name, with the ground-truth lines of the used
    classes of gt_labels_folder/name where the correction replaces or appends.  As in the reference, the `nonoise` branch cuts
    EVERY line to 83 characters (dtype "<U83", :148-149), a dropped image and an image left without a line get no file, and the
    lines are written as they were read.  A pseudo-label line outside `used_classes` would make the reference's line indices
    and the audit's object indices disagree silently: it is refused.  Returns the number of files written."""
    import os
    f = correction.flags
    os.makedirs(out_dir, exist_ok=True)
    written = 0
    for i, name in enumerate(audit.names):
        with open(os.path.join(det_folder, name), "r") as fh:
            pred_lines = fh.readlines()
        for k, line in enumerate(pred_lines):
            if line.strip().split(" ")[0] not in used_classes:
                raise ValueError("write_kitti_corrected_pseudo: line %d of %r is not of a used class; the reference would pair "
                                 "the audit's object indices with other lines" % (k, name))
        with open(os.path.join(gt_labels_folder, name), "r") as fh:
            gt_lines = [line for line in fh.readlines() if line.strip().split(" ")[0] in used_classes]
        _audit_sizes("write_kitti_corrected_pseudo", name, len(pred_lines), len(gt_lines), audit, i)
        if correction.dropped[i]:
            continue
        new_lines = pred_lines
        if f["remove_noise"]:
            new_lines = np.asarray(new_lines, dtype="<U83")
            repl = correction.replacements[i]
            if len(repl):
                new_lines[repl[:, 0]] = np.asarray(gt_lines, dtype="<U83")[repl[:, 1]]
            new_lines = list(new_lines)
        if f["remove_fds"] or f["high_precision"]:
            new_lines = list(np.asarray(pred_lines)[correction.kept[i]]) if len(correction.kept[i]) else []
        if len(correction.appended[i]):
            new_lines = new_lines + list(np.asarray(gt_lines)[correction.appended[i]])
        if len(new_lines) > 0:
            with open(os.path.join(out_dir, name), "w") as fh:
                fh.writelines(new_lines)
            written += 1
    return written


def write_bdd_corrected_pseudo(pred_items, bdd_data, out_dir, used_classes, audit, correction):
    """The pseudo_labels.json of `ThreeDproblem.corrected_pseudo` (3d.py:167-233): pred_items is the loaded pseudo-label json (or
    its path), bdd_data the loaded ground-truth json (or its path); the audit's images are pred_items, in order.  Per item the
    labels are kept, replaced by the ground-truth objects of the used classes, or appended to, as the correction says; a
    dropped image loses its entry.  As in the reference, an item whose selector is empty stays as it was, whatever the
    correction (:189).  A pseudo label outside `used_classes`, or an item order other than the audit's, would pair indices
    with other objects silently: both are refused.  The inputs are not modified.  Writes out_dir/pseudo_labels.json
    (json.dump, indent=4); returns the number of items written."""
    import copy
    import json
    import os
    if isinstance(pred_items, str):
        with open(pred_items, "r") as fh:
            pred_items = json.load(fh)
    if isinstance(bdd_data, str):
        with open(bdd_data, "r") as fh:
            bdd_data = json.load(fh)
    pred_items = copy.deepcopy(pred_items)
    f = correction.flags
    if [item["name"] for item in pred_items] != [str(nm) for nm in audit.names]:
        raise ValueError("write_bdd_corrected_pseudo: the items of the pseudo-label json are not the audit's images in its order")
    gt_im_names = np.asarray([item["name"] for item in bdd_data])
    for i, item in enumerate(pred_items):
        gt_i = np.where(item["name"] == gt_im_names)[0][0]
        for k, obj in enumerate(item["labels"]):
            if obj["category"] not in used_classes:
                raise ValueError("write_bdd_corrected_pseudo: label %d of %r is not of a used class; the reference would pair the "
                                 "audit's object indices with other labels" % (k, item["name"]))
        gt_objs = [copy.deepcopy(g) for g in bdd_data[gt_i]["labels"] if g["category"] in used_classes]
        _audit_sizes("write_bdd_corrected_pseudo", item["name"], len(item["labels"]), len(gt_objs), audit, i)
        if len(correction.selector[i]) > 0:
            if correction.dropped[i]:
                del pred_items[i]["labels"]
                continue
            new_items = list(item["labels"])
            for d, r in correction.replacements[i]:
                new_items[d] = gt_objs[r]
            if f["remove_fds"] or f["high_precision"]:
                new_items = [item["labels"][d] for d in correction.kept[i]]
            new_items += [gt_objs[r] for r in correction.appended[i]]
            pred_items[i]["labels"] = new_items
    out = [item for item in pred_items if "labels" in item]
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "pseudo_labels.json"), "w") as fh:
        json.dump(out, fh, indent=4)
    return len(out)
