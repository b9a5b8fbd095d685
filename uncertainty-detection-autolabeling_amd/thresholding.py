"""Thresholding: the middle step of the auto-label loop (reference uncertainty_analysis.py:44-327).  From the matched rows of a
validation run, find the weights that combine the selected uncertainties into one "is this detection wrong?" score, and the
threshold on that score that meets a budget of missed (`thr_cd`) or false detections.

  roc_objective         the reference's `roc_metrics` for P candidate weight vectors x K IoU thresholds in one device call
                        (`uda_thr_objective_np`: one sort per candidate, K curves on it)
  roc_metrics           one problem through the same kernel
  UncertOptimal         the reference's class: reads `optimal_params_*.txt` when present, else searches and writes it and
                        `optimal_thrs_*.txt`.  The reference searches with optuna or HEBO (stochastic, serial); here the search is
                        a seeded population search whose every round is one call of `objective`
  from_validate_records the columns UncertOptimal takes, from `writers.validate_records` or a validate_results.txt
  autolabel_verdict     the verdict of infer_model.py:753-755 on the image scores of `serve_score(..., "combo", ...)`
"""
import ast
import os

import numpy as np

from . import capi, hparams_config

MAX_N, MAX_U, MAX_K, MAX_P, MAX_G = capi.THR_MAX_N, capi.THR_MAX_U, capi.THR_MAX_THRS, capi.THR_MAX_P, capi.THR_MAX_G
DEFAULT_SEED = 20240521
DEFAULT_POPULATION, DEFAULT_ROUNDS = 256, 8          # up to 2048 + corners evaluations; never fewer than the reference's 1500
                                                     # unless a round fails to improve first


def _ptr(a):
    return a.ctypes.data_as(capi.C.c_void_p)


def _finite(a, what):
    if not np.isfinite(a).all():
        raise ValueError("%s holds NaN or inf" % what)
    return a


def check_problem(uncerts, ious, tp_class, iou_thrs, params, budget, group=None):
    """Contiguous arrays of the types the library takes; ValueError for a shape, a non-finite value or a limit."""
    uncerts = np.ascontiguousarray(np.asarray(uncerts, np.float64))
    if uncerts.ndim == 1:
        uncerts = uncerts[None]
    if uncerts.ndim != 2:
        raise ValueError("uncerts must be [U, N], got shape %s" % (uncerts.shape,))
    U, N = uncerts.shape
    if not 1 <= U <= MAX_U:
        raise ValueError("%d uncertainties: 1..%d are taken" % (U, MAX_U))
    if not 2 <= N <= MAX_N:
        raise ValueError("%d rows: 2..%d are taken" % (N, MAX_N))
    ious = np.ascontiguousarray(np.asarray(ious, np.float64).reshape(-1))
    tp = np.ascontiguousarray(np.asarray(tp_class).reshape(-1).astype(bool).astype(np.uint8))
    if ious.size != N or tp.size != N:
        raise ValueError("ious of %d rows and tp_class of %d for uncerts of %d" % (ious.size, tp.size, N))
    thrs = np.ascontiguousarray(np.asarray(iou_thrs, np.float64).reshape(-1))
    if not 1 <= thrs.size <= MAX_K:
        raise ValueError("%d IoU thresholds: 1..%d are taken" % (thrs.size, MAX_K))
    G = 0
    if group is not None:
        g = np.asarray(group).reshape(-1)
        if g.size != N:
            raise ValueError("group of %d rows for uncerts of %d" % (g.size, N))
        if not np.array_equal(g, np.round(g)) or g.min() < 0:
            raise ValueError("group ids must be whole numbers >= 0")
        group = np.ascontiguousarray(g.astype(np.int32))
        G = int(group.max()) + 1
    params = np.asarray(params, np.float64)
    if params.ndim == 1:
        params = params[None]
    params = np.ascontiguousarray(params)
    d = U * max(G, 1)
    if G > MAX_G:
        raise ValueError("%d groups: at most %d are taken" % (G, MAX_G))
    if params.ndim != 2 or params.shape[1] != d:
        raise ValueError("params must be [P, %d], got shape %s" % (d, params.shape))
    if not 1 <= params.shape[0] <= MAX_P:
        raise ValueError("%d candidates: 1..%d are taken" % (params.shape[0], MAX_P))
    budget = float(budget)
    if not 0.0 < budget < 1.0:
        raise ValueError("budget %r is not strictly between 0 and 1" % budget)
    _finite(uncerts, "uncerts"), _finite(ious, "ious"), _finite(thrs, "iou_thrs"), _finite(params, "params")
    return uncerts, ious, tp, thrs, params, budget, group, G


def roc_objective(uncerts, ious, tp_class, iou_thrs, params, fix_cd, budget, group=None, device=0):
    """The reference's `roc_metrics(sum(param * uncert), (ious >= iou_thr) * tp_class)` for every row of params [P, U] (or
    [P, U * G] with group [N] in 0..G-1: row i takes the weights params[p, group[i] * U : group[i] * U + U]) and every IoU
    threshold, on the device.  Returns (thr, rate, auc), float64 [P, K]; a problem with one label only gives (+inf, NaN, NaN)."""
    uncerts, ious, tp, thrs, params, budget, group, G = check_problem(uncerts, ious, tp_class, iou_thrs, params, budget, group)
    P, K = params.shape[0], thrs.size
    out = [np.zeros((P, K), np.float64) for _ in range(3)]
    lib = capi.load()
    rc = lib.uda_thr_objective_np(int(device), _ptr(uncerts), _ptr(ious), _ptr(tp), _ptr(group) if group is not None else None,
                                  uncerts.shape[1], uncerts.shape[0], G, _ptr(thrs), K, _ptr(params), P, int(bool(fix_cd)),
                                  budget, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]))
    capi.check(lib, None, rc, "uda_thr_objective_np")
    return tuple(out)


def roc_metrics(uncert, y_true, fix_cd=None, budget=None, device=0):
    """The reference's `roc_metrics(uncert, y_true)` (y_true 1 = a correct detection) for one problem: (thr, rate, auc).
    fix_cd / budget default to the hyper-parameters `thr_cd` / `thr_fpr_tpr`, the reference's module globals."""
    h = hparams_config.default_detection_configs()
    fix_cd = h.thr_cd if fix_cd is None else fix_cd
    budget = h.thr_fpr_tpr if budget is None else budget
    y = np.asarray(y_true).reshape(-1)
    thr, rate, auc = roc_objective(np.asarray(uncert, np.float64).reshape(1, -1), np.ones(y.size), y != 0, [0.5], [[1.0]], fix_cd,
                                   budget, device=device)
    return thr[0, 0], rate[0, 0], auc[0, 0]


def losses(rate):
    """`_f_x` per candidate: the mean over the IoU thresholds of rate * 100, a NaN rate counted as 1."""
    rate = np.asarray(rate, np.float64)
    return np.mean(np.where(np.isnan(rate), 1.0, rate) * 100, axis=1)


def population_search(evaluate, dim, population=DEFAULT_POPULATION, rounds=DEFAULT_ROUNDS, seed=DEFAULT_SEED, corners=()):
    """Deterministic minimisation over [0, 1]^dim.  evaluate(params [P, dim]) -> loss [P], one call per round.  Round 0: the
    given corners, then `population` points drawn uniformly; every further round `population` points from a box around the best
    so far, its side halved each round (1/2, 1/4, ...) and clipped to [0, 1].  Stops after `rounds` rounds or after a round that
    does not improve the best.  Returns (best params, best loss, all params, all losses); ties go to the earliest."""
    rng = np.random.default_rng(seed)
    first = [np.asarray(c, np.float64).reshape(1, dim) for c in corners] + [rng.uniform(0.0, 1.0, (population, dim))]
    tried = [np.concatenate(first)]
    loss = [np.asarray(evaluate(tried[0]), np.float64)]
    best = int(np.argmin(loss[0]))
    best_x, best_f = tried[0][best].copy(), loss[0][best]
    side = 1.0
    for _ in range(1, rounds):
        side /= 2
        lo, hi = np.clip(best_x - side / 2, 0.0, 1.0), np.clip(best_x + side / 2, 0.0, 1.0)
        x = rng.uniform(0.0, 1.0, (population, dim)) * (hi - lo) + lo
        f = np.asarray(evaluate(x), np.float64)
        tried.append(x)
        loss.append(f)
        i = int(np.argmin(f))
        if not f[i] < best_f:
            break
        best_x, best_f = x[i].copy(), f[i]
    return best_x, best_f, np.concatenate(tried), np.concatenate(loss)


def _settings(params):
    h = hparams_config.default_detection_configs().as_dict()
    src = params or {}
    return {k: src.get(k, h[k]) for k in ("thr_fpr_tpr", "thr_cd", "thr_iou_thrs", "thr_sel_uncert")}


def result_paths(source_path, params=None, added_name=""):
    """(optimal_params_*.txt, optimal_thrs_*.txt) as the reference names them (uncertainty_analysis.py:229-288)."""
    s = _settings(params)
    tail = ("cd" if s["thr_cd"] else "fd") + "_" + str(s["thr_fpr_tpr"]) + "_iou_" + str(np.min(s["thr_iou_thrs"])) + "_" + \
        str(np.max(s["thr_iou_thrs"])) + added_name + ".txt"
    return source_path + "/optimal_params_" + tail, source_path + "/optimal_thrs_" + tail


def write_values(path, values):
    with open(path, "w") as f:
        f.write(str(np.asarray(list(values), dtype="object")))


def read_values(path):
    """The reference's parser (uncertainty_analysis.py:323, infer_model.py reads the thresholds the same way)."""
    with open(path, "r") as f:
        return [float(x.strip("[]")) for x in f.read().split()]


class UncertOptimal:
    """Optimally combines the different uncertainties (reference class of the same name).  gt_classes: ground-truth class ids
    1..C per row (read when per_cls); tps_class: class == gt class; ious: IoU of each row's detection with its ground truth;
    uncert: list of U arrays [N].  params: model parameters carrying thr_fpr_tpr / thr_cd / thr_iou_thrs (the reference reads
    its defaults as module globals); objective: the batched evaluator, `roc_objective` on the device unless given."""

    def __init__(self, gt_classes=None, tps_class=None, ious=None, uncert=None, added_name="", source_path="", per_cls=False,
                 method="population", params=None, objective=None, population=DEFAULT_POPULATION, rounds=DEFAULT_ROUNDS,
                 seed=DEFAULT_SEED, device=0):
        if method != "population":
            raise ValueError("method %r is not available (optuna and hebo are not part of this package): use \"population\", "
                             "the seeded population search" % (method,))
        self.source_path = source_path
        self.added_name = added_name
        self.per_cls = per_cls
        self.gt_classes = gt_classes
        self.method = method
        self.settings = _settings(params)
        self.objective = objective or roc_objective
        self.population, self.rounds, self.seed, self.device = int(population), int(rounds), seed, device
        self.opt_thrs = None
        self.loss = None
        self.evaluated = None
        if tps_class is not None:
            self.tps_class = tps_class
            self.ious = ious
            self.uncert = uncert
            self.opt_params = [0, 0]

    def _columns(self):
        uncerts = np.stack([np.asarray(u, np.float64).reshape(-1) for u in self.uncert])
        group = None
        if self.per_cls:
            cls = np.asarray(self.gt_classes, np.float64).reshape(-1)
            if not np.array_equal(cls, np.round(cls)) or cls.min() < 1:
                raise ValueError("per_cls: gt_classes must be whole class ids >= 1")
            self.num_classes = int(cls.max())
            group = cls.astype(np.int32) - 1
        return uncerts, group

    def evaluate(self, params):
        """(thr, rate, auc) [P, K] of candidate rows through `objective`."""
        s = self.settings
        uncerts, group = self._columns()
        return self.objective(uncerts, self.ious, self.tps_class, s["thr_iou_thrs"], params, s["thr_cd"], s["thr_fpr_tpr"],
                              group=group, device=self.device)

    def _extract_optimal_params(self, break_iter=10):
        """Searches the weights, writes optimal_params_*.txt and optimal_thrs_*.txt.  break_iter belongs to the reference's HEBO
        loop and is not read."""
        uncerts, _ = self._columns()
        U = uncerts.shape[0]
        dim = U * (self.num_classes if self.per_cls else 1)
        reps = dim // U
        corners = [np.tile(np.eye(U)[j], reps) for j in range(U)] + [np.ones(dim)]
        best, f, tried, loss = population_search(lambda x: losses(self.evaluate(x)[1]), dim, self.population, self.rounds,
                                                 self.seed, corners)
        self.opt_params = [float(v) for v in best]
        self.loss, self.evaluated = float(f), (tried, loss)
        self.opt_thrs = [float(v) for v in self.evaluate(best[None])[0][0]]
        p_path, t_path = result_paths(self.source_path, self.settings, self.added_name)
        write_values(p_path, self.opt_params)
        write_values(t_path, self.opt_thrs)

    def get_optimal_uncertainty(self, break_iter=10):
        """Reads the optimal weight vector if its file exists, else determines and writes it."""
        p_path, t_path = result_paths(self.source_path, self.settings, self.added_name)
        if os.path.exists(p_path):
            self.opt_params = read_values(p_path)
            if os.path.exists(t_path):
                self.opt_thrs = read_values(t_path)
        else:
            self._extract_optimal_params(break_iter)
        return self.opt_params


def calc_iou_np(gt_boxes, pred_boxes):
    """utils_box.calc_iou_np (:56-90) on float64 [N, 4] y1 x1 y2 x2 rows; 0 where the union is empty."""
    g, p = np.asarray(gt_boxes, np.float64).reshape(-1, 4), np.asarray(pred_boxes, np.float64).reshape(-1, 4)
    ya, xa = np.maximum(g[:, 0], p[:, 0]), np.maximum(g[:, 1], p[:, 1])
    yb, xb = np.minimum(g[:, 2], p[:, 2]), np.minimum(g[:, 3], p[:, 3])
    inter = np.maximum(0.0, xb - xa) * np.maximum(0.0, yb - ya)
    union = np.abs(g[:, 3] - g[:, 1]) * np.abs(g[:, 2] - g[:, 0]) + np.abs(p[:, 3] - p[:, 1]) * np.abs(p[:, 2] - p[:, 0]) - inter
    return np.divide(inter, union, out=np.zeros_like(inter), where=union != 0)


def relativize_uncert(pred_boxes, box_uncert):
    """utils_box.relativize_uncert (:279-292): sigma of y1, x1, y2, x2 over height, width, height, width."""
    b, u = np.asarray(pred_boxes, np.float64), np.asarray(box_uncert, np.float64)
    w, h = b[:, 3] - b[:, 1], b[:, 2] - b[:, 0]
    return u / np.stack([h, w, h, w], 1)


def from_validate_records(records, params, calib=False):
    """The columns of `MainUncertViz.__init__` / `_read_predictions` (uncertainty_analysis.py:366-392, :882-918) from the
    records of `writers.validate_records`, or from the path of a validate_results.txt: rows whose ground-truth box overlaps
    its detection (IoU > 0) only.  Returns a dict: gt_classes, tps_class, ious, uncert (the list `thr_sel_uncert` selects:
    entropy, then the mean relative aleatoric sigma; the calibrated columns when calib), pred_classes, image_names."""
    if isinstance(records, (str, os.PathLike)):
        with open(records, "r") as f:
            records = [ast.literal_eval(line.replace("inf", "2e308")) for line in f if line.strip()]
    if not records:
        raise ValueError("no validation records")
    gt_boxes = np.asarray([r["gt_bbox"] for r in records], np.float64)
    boxes = np.asarray([r["bbox"] for r in records], np.float64)
    ious = calc_iou_np(gt_boxes, boxes)
    hit = ious > 0.0

    def col(key):
        if key not in records[0]:
            raise ValueError("the validation records have no %r (thr_sel_uncert %r, calib=%r)" % (key, sel, calib))
        return np.asarray([r[key] for r in records], np.float64)[hit]

    sel = str(params.get("thr_sel_uncert", "ENTALBOX"))
    ent_key = "%s_entropy" % params.get("calib_method_class") if calib else "entropy"
    al_key = "%s_albox" % params.get("calib_method_box") if calib else "uncalib_albox"
    uncert = []
    if "ENT" in sel:
        uncert.append(col(ent_key))
    if "ALBOX" in sel:
        uncert.append(np.mean(relativize_uncert(boxes[hit], col(al_key)), axis=-1))
    if not uncert:
        raise ValueError("thr_sel_uncert %r selects neither ENT nor ALBOX" % sel)
    pred_classes, gt_classes = col("class"), col("gt_class")
    return {"gt_classes": gt_classes, "tps_class": pred_classes == gt_classes, "ious": ious[hit], "uncert": uncert,
            "pred_classes": pred_classes, "image_names": [r["image_name"] for r, h in zip(records, hit) if h]}


def autolabel_verdict(image_scores, opt_thrs):
    """infer_model.py:753-755: an image is auto-labeled iff every kept detection's combined score is below mean(opt_thrs).
    image_scores: what `serve_score(images, "combo", min_score, opt_params)` returns with the reduce `max` - (components
    [n, 1], count [n], ...) - or the two arrays themselves.  An image with no kept row is auto-labeled (np.all of nothing)."""
    comp, count = image_scores[0], image_scores[1]
    top = np.asarray(comp, np.float64).reshape(len(count), -1)[:, 0]
    return (np.asarray(count) == 0) | (top < np.mean(np.asarray(opt_thrs, np.float64)))
