"""The teacher's pseudo-labelling step of the reference's semi-supervised loop (src/SSL_stac.py:202-642: `STAC.predict_teacher`
-> `STAC.score_image` -> `write_KITTI_pseudo_gt_txt` / `write_BDD_pseudo_gt_json`) without the text file in between.

The reference serves the unlabeled images with min_score 0.1, writes one dict per detection to prediction_data.txt, parses every
line back, gives each of an image's first 99 detections one uncertainty value, filters by `tau`, normalises the values with the
minimum and maximum over the whole dataset, filters again and writes the survivors as ground truth.  Here the per-row value, the
99-row cap, the `tau` filter and the per-image min / max run on the device, on the detections resident in a handle
(`ServingDriver.pseudo_rows` / `serve_pseudo_labels`, C entry point uda_pseudo_rows) or on host arrays (`select_detections`,
uda_pseudo_rows_np); the host keeps the candidate records - a few dozen per image - and does the dataset-wide part.

  resolve_selection     STAC's substring grammar -> `Selection` (descriptor, invert, gate, final rule)
  PseudoLabelSet        accumulator over batches + the second half of score_image (:543-642); picklable, `merge` for shards
  select_detections     the same kernels on host columns (calibrated strategies, gathered multi-GPU batches)
  write_kitti_pseudo_gt / write_bdd_pseudo_gt   the reference's files, byte for byte

Deviations from the file route: the device reads the unrounded float32 columns where the file holds them rounded;
every branch is capped at `max_rows` rows per image, where the reference's multi-column branches slice the list of columns
instead of the rows: on an image with 100 written rows they raise IndexError when it has a survivor, and otherwise let the 100th
row's value into the dataset-wide min / max, which this path does not.
"""
import ctypes as C
import json
import os

import numpy as np

from . import active_learning as al
from . import capi

MAX_ROWS = 99                         # STAC.score_image: max_detections_per_image
RECORD_DTYPE = np.dtype([("image", "<i4"), ("row", "<i4"), ("box", "<f4", (4,)), ("det_score", "<f4"), ("cls", "<i4"), ("v", "<f8")])
assert RECORD_DTYPE.itemsize == 40    # uda_pseudo_record_t
RULES = ("combo", "alluncert", "sigmoid", "tau")


class Selection(al.Strategy):
    """A resolved selection strategy: the descriptor of `active_learning.Strategy` (components, columns, calibrated) and
    invert: v = 1 / mean of the 2 or 3 components (else the one component itself);
    gate: a row is a candidate iff v > tau (else iff det_score > tau);
    rule: what `PseudoLabelSet.finalize` applies - "combo" (0 < normalised <= mean(opt_thrs)), "alluncert" (normalised > tau),
    "sigmoid" (epuncert / ental: the det_score filter alone), "tau" (the single-column branch: v > tau, no normalisation);
    activate_pseudoscore: the score is returned and written."""

    def __init__(self, name, components, columns, calibrated, invert, gate, rule, activate_pseudoscore):
        al.Strategy.__init__(self, name, components, False, columns, calibrated, None)
        assert rule in RULES
        self.invert, self.gate, self.rule = int(invert), int(gate), rule
        self.activate_pseudoscore = bool(activate_pseudoscore)

    def __repr__(self):
        return "Selection(%r, %r, invert=%d, gate=%d, %s)" % (self.name, self.components, self.invert, self.gate, self.rule)


def resolve_selection(strategy, params, opt_params=None):
    """`STAC.selection_strategy` -> `Selection`, branch for branch in the order of score_image's row loop (:387-528): `combo`;
    `alluncert`; `epuncert`; `ental`; otherwise the key add_mode + strategy.split("_")[-1] of a file line, det_score when the
    line would not hold it.  All tests are substring tests.  params as in `active_learning.resolve_strategy`.

    Where STAC and the active-learning loop differ: STAC has no `sota` branch (the word falls through to the last branch and
    there to det_score); `combo` beside another branch word is served as `combo` (STAC's accumulator is sized by the other
    word but read by position, which works); there is no mean / max over the image."""
    s = str(strategy)
    t = al._Terms(s, al._emitted(params))
    if "combo" in s:
        comps, invert, gate, rule = t.combo(opt_params), 0, 0, "combo"
    elif "alluncert" in s:
        comps, invert, gate, rule = t.alluncert(), 1, 0, "alluncert"
    elif "epuncert" in s:
        comps, invert, gate, rule = t.epuncert(), 1, 0, "sigmoid"
    elif "ental" in s:
        comps, invert, gate, rule = t.ental(), 1, 0, "sigmoid"
    else:
        comps, invert, gate, rule = t.single(), 0, 1, "tau"
    return Selection(s, comps, t.columns, t.calibrated(), invert, gate, rule, "pseudoscore" in s)


def _check_tau(tau):
    tau = float(tau)
    if not tau >= 0.0:
        raise ValueError("tau must not be negative, got %r" % (tau,))
    return tau


class PseudoLabelSet:
    """The candidates of a dataset, accumulated over its batches, and the second half of `STAC.score_image` (:543-642).

    selection: a `Selection`; tau: STAC's `tau`; opt_thrs: the optimal thresholds of the thresholding step (`combo` only:
    their mean is the upper bound).  Holds plain lists and arrays: it pickles, and `merge` appends another set's images
    (the shards of `dist.py`, in rank order)."""

    def __init__(self, selection, tau, opt_thrs=None):
        if not isinstance(selection, Selection):
            raise TypeError("PseudoLabelSet takes a Selection (resolve_selection)")
        self.selection, self.tau = selection, _check_tau(tau)
        if selection.rule == "combo" and (opt_thrs is None or len(opt_thrs) < 1):
            raise ValueError("strategy %r needs opt_thrs (the thresholding step's optimal thresholds)" % selection.name)
        self.opt_thrs = None if opt_thrs is None else [float(x) for x in opt_thrs]
        self.names, self._cls, self._boxes, self._v = [], [], [], []
        self.min, self.max = float("inf"), float("-inf")
        self.n_images = 0

    def add(self, names, result, boxes=None):
        """names: the batch's image names; result: (records, minmax [n, 2], kept [n], cand [n]) of `pseudo_rows` /
        `select_detections`.  boxes: optional [n, M, 4] columns to take the candidates' boxes from (host callers, whose
        columns are float64) instead of the records' float32 ones.  Returns the number of images with a candidate."""
        rec, minmax, kept, cand = result
        names = list(names)
        if len(names) != len(cand):
            raise ValueError("%d names for %d images" % (len(names), len(cand)))
        rec = np.asarray(rec)
        if rec.dtype != RECORD_DTYPE or rec.ndim != 1 or len(rec) != int(np.sum(cand)):
            raise ValueError("records must be %d rows of RECORD_DTYPE" % int(np.sum(cand)))
        for lo, hi in np.asarray(minmax, np.float64).reshape(-1, 2).tolist():
            self.min = min(self.min, lo)              # (an image where no row takes part reports +inf, -inf: neutral)
            self.max = max(self.max, hi)
        self.n_images += len(names)
        off, added = 0, 0
        for i, k in enumerate(np.asarray(cand).tolist()):
            if not k:
                continue
            r = rec[off:off + k]
            off += k
            if not (r["image"] == i).all():
                raise ValueError("records are not in image order")
            self.names.append(names[i])
            self._cls.append(r["cls"].astype(np.float64))
            self._boxes.append(r["box"].astype(np.float64) if boxes is None else np.asarray(boxes)[i, r["row"], :4].astype(np.float64))
            self._v.append(r["v"].astype(np.float64))
            added += 1
        return added

    def merge(self, other):
        if other.selection.name != self.selection.name or other.tau != self.tau or other.opt_thrs != self.opt_thrs:
            raise ValueError("merge: the sets were built with different strategy, tau or opt_thrs")
        self.names += other.names
        self._cls += other._cls
        self._boxes += other._boxes
        self._v += other._v
        self.min, self.max = min(self.min, other.min), max(self.max, other.max)
        self.n_images += other.n_images
        return self

    def __len__(self):
        return len(self.names)

    def _normalize(self, v):
        """minmax_normalize (:322-341) with the minimum and maximum over everything added."""
        spread = self.max - self.min
        if not spread > 0:
            return np.zeros_like(v)
        with np.errstate(all="ignore"):
            return (v - self.min) / spread

    def finalize(self):
        """-> (pred_imgs_names, pred_classes, pred_boxes[, pseudo_score]) as `STAC.score_image` returns them: an array of
        names, per image an array of class ids (float64), of boxes [k, 4] (y1 x1 y2 x2) and - under a `pseudoscore` strategy -
        of scores.  Images without a survivor are dropped."""
        sel, rule = self.selection, self.selection.rule
        names, classes, boxes, scores = [], [], [], []
        bound = None if rule != "combo" else np.mean(self.opt_thrs)
        for name, c, b, v in zip(self.names, self._cls, self._boxes, self._v):
            # every candidate passed the device's filter (det_score > tau, or v > tau): the sigmoid filter multiplies by 1
            s = v if rule == "tau" else self._normalize(v)
            if rule == "combo":
                keep = (s <= bound) * (s > 0)
            elif rule == "alluncert":
                keep = s > self.tau
            else:
                keep = np.ones(len(s), bool)
            if not keep.any():
                continue
            names.append(name)
            classes.append(c[keep])
            boxes.append(b[keep])
            scores.append(s[keep])
        out = (np.asarray(names), classes, boxes)
        return out + (scores,) if sel.activate_pseudoscore else out


def select_detections(columns, strategy, tau, min_score=0.1, params=None, opt_params=None, num_classes=None, max_rows=MAX_ROWS,
                      device=0, as_float32=False):
    """`pseudo_rows` on host arrays, through the same kernels in float64 (uda_pseudo_rows_np): for the calibrated strategies
    - the columns the calibrators return already are on the host - and for callers that hold detections of their own.

    columns, strategy (a string or a `Selection`), params, num_classes, as_float32: as `active_learning.score_detections`
    takes them; box columns may hold zero sides (IEEE: inf / NaN values), the other columns must be finite.
    Returns (records [K] RECORD_DTYPE in (image, rank) order, minmax [n, 2] float64, kept [n] int32, cand [n] int32)."""
    tau = _check_tau(tau)
    strategy, arrays, n, M, mcw, num_classes = al.detection_columns(columns, strategy, resolve_selection, params, opt_params, num_classes,
                                                                    as_float32)
    if int(max_rows) < 1:
        raise ValueError("max_rows must be at least 1")
    rec = np.zeros((n * min(M, int(max_rows)),), RECORD_DTYPE)
    minmax = np.zeros((n, 2), np.float64)
    kept = np.zeros((n,), np.int32)
    cand = np.zeros((n,), np.int32)
    K = C.c_int64()
    lib = capi.load()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    desc = strategy.desc()
    fn, what = (lib.uda_pseudo_rows_np_f32, "uda_pseudo_rows_np_f32") if as_float32 else (lib.uda_pseudo_rows_np, "uda_pseudo_rows_np")
    al.raise_from_rc(fn(int(device), C.byref(desc), float(min_score), *[p(a) for a in arrays], n, M, num_classes, mcw, strategy.invert,
                        strategy.gate, tau, int(max_rows), p(rec), C.byref(K), p(minmax), p(kept), p(cand)), lib, what)
    return rec[:K.value].copy(), minmax, kept, cand


def _class_names(label_map):
    """dataset name ("kitti", "bdd"), path containing it, or {id: name} -> {id: name} (dataset_data)."""
    from . import dataset_data
    if isinstance(label_map, str) and label_map.lower() not in dataset_data._LABEL_MAPS:
        lm = dataset_data.get_dataset_data(label_map)[0]
        if not lm:
            raise KeyError(label_map)
        return lm
    return dataset_data.get_label_map(label_map.lower() if isinstance(label_map, str) else label_map)


def _named(selected, label_map):
    """The tuple of `finalize` with the class ids turned into names (`select_classes[int(c) - 1]`, :1025-1028)."""
    names = _class_names(label_map)
    pseudo = selected[3] if len(selected) > 3 else None
    classes = [[names[int(c)] for c in c_im] for c_im in selected[1]]
    return selected[0], classes, selected[2], pseudo


def write_kitti_pseudo_gt(output_dir, selected, label_map="kitti"):
    """`STAC.write_KITTI_pseudo_gt_txt` (:202-237): one <image stem>.txt per image, one line per detection - the capitalised
    class name, dummy KITTI fields, x1 y1 x2 y2, and -10 or the rounded pseudo score (when `selected` carries one).
    selected: what `PseudoLabelSet.finalize` returned.  Returns n_dets."""
    img_names, classes, boxes, pseudo = _named(selected, label_map)
    n_dets = 0
    os.makedirs(output_dir, exist_ok=True)
    for k, name in enumerate(img_names):
        with open(os.path.join(output_dir, "%s.txt" % str(name).split(".")[0]), "w") as f:
            for j, (cname, box) in enumerate(zip(classes[k], boxes[k])):
                last = "-10" if pseudo is None else "%s" % (np.round(pseudo[k][j], 2),)
                f.write("%s 0.0 0 -10 %s %s %s %s 0.0 0.0 0.0 0.0 0.0 0.0 %s\n" % (cname.capitalize(), box[1], box[0], box[3], box[2], last))
                n_dets += 1
    return n_dets


def write_bdd_pseudo_gt(output_dir, selected, label_map="bdd"):
    """`STAC.write_BDD_pseudo_gt_json` (:239-300): pseudo_labels.json, json.dump(..., indent=4).  Returns n_dets."""
    img_names, classes, boxes, pseudo = _named(selected, label_map)
    n_dets = 0
    os.makedirs(output_dir, exist_ok=True)
    pseudo_gt = []
    for k, name in enumerate(img_names):
        image_data = {"name": str(name), "attributes": {"weather": "overcast", "timeofday": "daytime", "scene": "city street"},
                      "timestamp": 10000, "labels": []}
        for j, (cname, box) in enumerate(zip(classes[k], boxes[k])):
            label = {"id": str(j), "attributes": {"occluded": False, "truncated": False, "trafficLightColor": "NA"}, "category": cname,
                     "box2d": {"x1": float(box[1]), "y1": float(box[0]), "x2": float(box[3]), "y2": float(box[2])}}
            if pseudo is not None:
                label["pseudo_score"] = float(np.round(pseudo[k][j], 2))
            image_data["labels"].append(label)
            n_dets += 1
        pseudo_gt.append(image_data)
    with open(os.path.join(output_dir, "pseudo_labels.json"), "w") as f:
        json.dump(pseudo_gt, f, indent=4)
    return n_dets
