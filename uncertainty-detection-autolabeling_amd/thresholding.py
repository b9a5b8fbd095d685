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
  thr_report            the judgement after the search (uncertainty_analysis.py:398-500, :517-749): per score column, IoU threshold
                        and row segment (all rows, each ground-truth class) the curve, the moments behind `calc_jsd` and the
                        removal counts in one device call (`uda_thr_report_np`); `save_thr_performance` (thr_metrics_*.txt and
                        the table), `collect_thresh_results`, `clsoptfix_params` (the `_clsoptfix` rule), `threshold_analysis`
                        (the whole sequence of `MainUncertViz.__init__`)
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


# ------------------------------------------------------------------------------------------------ the thresholding report
# The judgement the reference makes right after the search (MainUncertViz.__init__ / _save_thr_performance /
# _collect_thresh_results, uncertainty_analysis.py:398-500, :517-749, with calc_jsd, utils_extra.py:25-36): per score column, IoU
# threshold and segment of rows (all rows, one ground-truth class) the curve, the moments behind the JSD and the removal counts
# come from one device call (`uda_thr_report_np`); the combinations, the JSD itself, the roundings and the texts are formed here.
MAX_S, MAX_SEGS = capi.THR_REPORT_MAX_S, capi.THR_REPORT_MAX_SEGS


def calc_jsd(dist_1, dist_2):
    """utils_extra.calc_jsd (:25-36): the Jensen-Shannon distance of the normal densities fitted to two samples, on 1000 points
    over the union of their +-3 sigma ranges.  NaN for an empty sample or a zero std."""
    import scipy.spatial.distance
    import scipy.stats
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mean_1, std_1 = np.mean(dist_1), np.std(dist_1)
            mean_2, std_2 = np.mean(dist_2), np.std(dist_2)
    return jsd_from_moments(mean_1, std_1, mean_2, std_2, _scipy=(scipy.stats, scipy.spatial.distance))


def jsd_from_moments(mean1, std1, mean2, std2, _scipy=None):
    """calc_jsd from the two means and (population) standard deviations.  An empty sample (mean NaN) or a zero std gives NaN, as
    the reference's expression does (scipy's pdf is NaN for scale <= 0, and NaN runs through linspace and jensenshannon)."""
    if not (std1 > 0 and std2 > 0 and np.isfinite(mean1) and np.isfinite(mean2) and np.isfinite(std1) and np.isfinite(std2)):
        return np.float64(np.nan)
    if _scipy is None:
        import scipy.spatial.distance
        import scipy.stats
        _scipy = (scipy.stats, scipy.spatial.distance)
    stats, distance = _scipy
    x = np.linspace(min(mean1 - 3 * std1, mean2 - 3 * std2), max(mean1 + 3 * std1, mean2 + 3 * std2), 1000)
    # (norm.pdf with loc and scale is what the frozen norm(loc, scale).pdf of the reference calls, without building the object)
    return distance.jensenshannon(stats.norm.pdf(x, loc=mean1, scale=std1), stats.norm.pdf(x, loc=mean2, scale=std2))


def segments_by_class(gt_classes, num_classes=None):
    """(order, seg_lo, seg_hi): the stable order of the rows by ground-truth class id 1..C and the half-open ranges of the ordered
    rows - "all" first, then classes 1..C; a class nobody has is an empty range.  num_classes defaults to the largest id."""
    cls = np.asarray(gt_classes, np.float64).reshape(-1)
    if cls.size == 0 or not np.array_equal(cls, np.round(cls)) or cls.min() < 1:
        raise ValueError("gt_classes must be whole class ids >= 1")
    C = int(cls.max()) if num_classes is None else int(num_classes)
    if cls.max() > C:
        raise ValueError("class id %d above num_classes %d" % (int(cls.max()), C))
    ids = cls.astype(np.int64)
    order = np.argsort(ids, kind="stable")
    ends = np.cumsum(np.bincount(ids, minlength=C + 1)[1:])
    seg_lo = np.concatenate([[0], [0], ends[:-1]]).astype(np.int32)
    seg_hi = np.concatenate([[cls.size], ends]).astype(np.int32)
    return order, seg_lo, seg_hi


def check_report_problem(scores, ious, tp_class, iou_thrs, budget, seg_lo, seg_hi):
    """Contiguous arrays of the types `uda_thr_report_np` takes; ValueError for a shape, a non-finite value or a limit."""
    scores = np.ascontiguousarray(np.asarray(scores, np.float64))
    if scores.ndim == 1:
        scores = scores[None]
    if scores.ndim != 2:
        raise ValueError("scores must be [S, N], got shape %s" % (scores.shape,))
    S, N = scores.shape
    if not 1 <= S <= MAX_S:
        raise ValueError("%d score columns: 1..%d are taken" % (S, MAX_S))
    if not 2 <= N <= MAX_N:
        raise ValueError("%d rows: 2..%d are taken" % (N, MAX_N))
    ious = np.ascontiguousarray(np.asarray(ious, np.float64).reshape(-1))
    tp = np.ascontiguousarray(np.asarray(tp_class).reshape(-1).astype(bool).astype(np.uint8))
    if ious.size != N or tp.size != N:
        raise ValueError("ious of %d rows and tp_class of %d for scores of %d" % (ious.size, tp.size, N))
    thrs = np.ascontiguousarray(np.asarray(iou_thrs, np.float64).reshape(-1))
    if not 1 <= thrs.size <= MAX_K:
        raise ValueError("%d IoU thresholds: 1..%d are taken" % (thrs.size, MAX_K))
    lo, hi = np.asarray(seg_lo).reshape(-1), np.asarray(seg_hi).reshape(-1)
    if lo.size != hi.size or not 1 <= lo.size <= MAX_SEGS:
        raise ValueError("%d / %d segment bounds: 1..%d pairs are taken" % (lo.size, hi.size, MAX_SEGS))
    if not (np.array_equal(lo, np.round(lo)) and np.array_equal(hi, np.round(hi))) or (lo < 0).any() or (hi < lo).any() \
            or (hi > N).any():
        raise ValueError("a segment is not a range [lo, hi) inside [0, %d]" % N)
    budget = float(budget)
    if not 0.0 < budget < 1.0:
        raise ValueError("budget %r is not strictly between 0 and 1" % budget)
    _finite(scores, "scores"), _finite(ious, "ious"), _finite(thrs, "iou_thrs")
    return scores, ious, tp, thrs, budget, np.ascontiguousarray(lo.astype(np.int32)), np.ascontiguousarray(hi.astype(np.int32))


def report_np(scores, ious, tp_class, iou_thrs, fix_cd, budget, seg_lo, seg_hi, device=0):
    """The raw device call: (roc [B, S, K, 3] thr / rate / auc, n_label [B, K, 2] int64, moments [B, S, K, 2, 2] (correct | wrong)
    x (sum, m2), removed [B, S, K, 3] int64) of `uda_thr_report_np` for the row ranges [seg_lo[b], seg_hi[b])."""
    scores, ious, tp, thrs, budget, lo, hi = check_report_problem(scores, ious, tp_class, iou_thrs, budget, seg_lo, seg_hi)
    (S, N), K, B = scores.shape, thrs.size, lo.size
    roc, n_label = np.zeros((B, S, K, 3), np.float64), np.zeros((B, K, 2), np.int64)
    moments, removed = np.zeros((B, S, K, 2, 2), np.float64), np.zeros((B, S, K, 3), np.int64)
    lib = capi.load()
    rc = lib.uda_thr_report_np(int(device), _ptr(scores), _ptr(ious), _ptr(tp), N, S, _ptr(thrs), K, _ptr(lo), _ptr(hi), B,
                               int(bool(fix_cd)), budget, _ptr(roc), _ptr(n_label), _ptr(moments), _ptr(removed))
    capi.check(lib, None, rc, "uda_thr_report_np")
    return roc, n_label, moments, removed


class ThrReport:
    """What `thr_report` returns.  Arrays over [B segments, S columns, K thresholds] unless noted: thr, rate, auc; n_correct,
    n_wrong [B, K]; mean, std [B, S, K, 2] of the correct (0) and the wrong (1) rows, NaN for an empty subset; correctly_removed,
    falsely_removed, falsely_remaining.  order / seg_lo / seg_hi: the row order the call used and the segments' ranges in it."""

    def __init__(self, roc, n_label, moments, removed, order, seg_lo, seg_hi):
        self.thr, self.rate, self.auc = roc[..., 0], roc[..., 1], roc[..., 2]
        self.n_correct, self.n_wrong = n_label[..., 0], n_label[..., 1]
        n = n_label[:, None, :, :].astype(np.float64)
        with np.errstate(all="ignore"):
            self.mean = moments[..., 0] / n
            self.std = np.sqrt(moments[..., 1] / n)
        self.sum, self.m2 = moments[..., 0], moments[..., 1]
        self.correctly_removed, self.falsely_removed, self.falsely_remaining = removed[..., 0], removed[..., 1], removed[..., 2]
        self.order, self.seg_lo, self.seg_hi = order, seg_lo, seg_hi
        self._jsd = None

    @property
    def jsd(self):
        """The reference's `np.nan_to_num(calc_jsd(u[correct], u[~correct]))`."""
        if self._jsd is None:
            import scipy.spatial.distance
            import scipy.stats
            sc = (scipy.stats, scipy.spatial.distance)
            out = np.zeros(self.thr.shape, np.float64)
            for i in np.ndindex(*out.shape):
                m, s = self.mean[i], self.std[i]
                out[i] = np.nan_to_num(jsd_from_moments(m[0], s[0], m[1], s[1], _scipy=sc))
            self._jsd = out
        return self._jsd

    @property
    def auc100(self):
        return np.nan_to_num(self.auc) * 100

    @property
    def fdcd(self):
        """FD@CD / CD@FD in percent: (1 - rate) * 100, 0 where the rate is NaN."""
        with np.errstate(invalid="ignore"):
            return np.where(np.isnan(self.rate), 0.0, (1 - self.rate) * 100)

    def jsd_mean(self):
        return np.mean(self.jsd, axis=-1)

    def auc_mean(self):
        return np.mean(self.auc100, axis=-1)

    def fdcd_mean(self):
        return np.mean(self.fdcd, axis=-1)


def thr_report(scores, ious, tp_class, iou_thrs, fix_cd, budget, gt_classes=None, num_classes=None, device=0, report=None):
    """The report of S ready score columns [S, N] over all rows (segment 0) and, with gt_classes, over every ground-truth class
    1..C (segments 1..C; rows are put in class order for the call, stably).  report: a stand-in for `report_np` with its
    signature (tests inject the numpy mirror)."""
    scores = np.asarray(scores, np.float64)
    if scores.ndim == 1:
        scores = scores[None]
    N = scores.shape[-1]
    ious, tp = np.asarray(ious, np.float64).reshape(-1), np.asarray(tp_class).reshape(-1).astype(bool)
    if gt_classes is None:
        order, lo, hi = np.arange(N), np.zeros(1, np.int32), np.full(1, N, np.int32)
    else:
        order, lo, hi = segments_by_class(gt_classes, num_classes)
        if order.size != N:
            raise ValueError("gt_classes of %d rows for scores of %d" % (order.size, N))
        if ious.size != N or tp.size != N:
            raise ValueError("ious of %d rows and tp_class of %d for scores of %d" % (ious.size, tp.size, N))
        scores, ious, tp = scores[:, order], ious[order], tp[order]
    out = (report or report_np)(scores, ious, tp, iou_thrs, fix_cd, budget, lo, hi, device=device)
    return ThrReport(*out, order, lo, hi)


def _combine(params, uncerts):
    """`sum(param * uncert ...)`: 0 + p0 * u0 + p1 * u1 ..., every product and sum rounded, left to right."""
    return sum(p * u for p, u in zip(params, uncerts))


def combine_per_class(uncerts, classes, params, num_classes):
    """The per-class combination of `MainUncertViz.__init__` (:423-444): class i + 1 takes the weights params[i * U : i * U + U],
    the running index advancing for every class."""
    collected = [np.array(u, np.float64) for u in uncerts]
    classes = np.asarray(classes)
    n_iter = 0
    for i in range(num_classes):
        for j in range(len(collected)):
            collected[j][classes == i + 1] *= params[n_iter]
            n_iter += 1
    return np.sum(collected, axis=0)


def _thr_metrics_path(source_path, s, added_name):
    return source_path + "/thr_metrics_" + ("cd" if s["thr_cd"] else "fd") + "_" + str(s["thr_fpr_tpr"]) + "_iou_" + \
        str(np.min(s["thr_iou_thrs"])) + "_" + str(np.max(s["thr_iou_thrs"])) + added_name + ".txt"


def save_thr_performance(source_path, params, selected_uncert, opt_uncert, tps_class, ious, gt_classes=None, opt_params=None,
                         label_map=None, added_name="", device=0, report=None):
    """`_save_thr_performance` (:517-732) without the figure: writes thr_metrics_*.txt under the reference's name and returns
    fprs_opt, the mean FD@CD / CD@FD of opt_uncert over the IoU thresholds; with opt_params (and gt_classes) returns
    (fprs_opt, table_data), the rows of the reference's per-class table.  The class rows use the reference's own per-class
    combination: the global weights when len(opt_params) == U, else the next U weights per class, the running index advancing only
    for classes that have rows (:576-595).  An odd number of IoU thresholds with opt_params raises ValueError (the reference's
    header rows have unequal lengths there and its np.asarray(table_data) raises)."""
    s = _settings(params)
    thrs = [float(t) for t in s["thr_iou_thrs"]]
    K, U = len(thrs), len(selected_uncert)
    metric = ("FD@CD" if s["thr_cd"] else "CD@FD") + str(int(s["thr_fpr_tpr"] * 100))
    cols = [np.asarray(u, np.float64).reshape(-1) for u in selected_uncert] + [np.asarray(opt_uncert, np.float64).reshape(-1)]
    tps_class, ious = np.asarray(tps_class).reshape(-1).astype(bool), np.asarray(ious, np.float64).reshape(-1)
    classes = None
    if opt_params is not None:
        if gt_classes is None:
            raise ValueError("opt_params: the per-class table needs gt_classes")
        if K % 2:
            raise ValueError("%d IoU thresholds: the reference's table has header rows of unequal lengths for an odd number" % K)
        classes = np.asarray(gt_classes, np.float64).reshape(-1)
        num_classes = int(max(classes))
        if len(opt_params) != U and len(opt_params) < U * len(np.unique(classes)):
            raise ValueError("%d opt_params for %d uncertainties and %d classes with rows" % (len(opt_params), U,
                                                                                           len(np.unique(classes))))
        cls_col = np.zeros(cols[0].size, np.float64)            # one column: the classes' rows are disjoint
        n_iter = 0
        for i in range(num_classes):
            sel = np.where(classes == i + 1)[0]
            if len(sel) > 0:
                per = [c[sel] for c in cols[:U]]
                if len(opt_params) == U:
                    cls_col[sel] = _combine(opt_params, per)
                else:
                    for j in range(U):
                        per[j] = per[j] * opt_params[n_iter]
                        n_iter += 1
                    cls_col[sel] = np.sum(per, axis=0)
        cols.append(cls_col)
    rep = thr_report(np.stack(cols), ious, tps_class, thrs, s["thr_cd"], s["thr_fpr_tpr"], gt_classes=classes, device=device,
                     report=report)
    jsd, auc, fdcd = rep.jsd, rep.auc100, rep.fdcd
    jsds_orig, aucs_orig, fprs_orig = jsd[0, :U], auc[0, :U], fdcd[0, :U]
    jsds_opt, aucs_opt, fprs_opt = jsd[0, U], auc[0, U], fdcd[0, U]
    table_data = None
    if opt_params is not None:
        has = (rep.seg_hi[1:] > rep.seg_lo[1:])[:, None]
        class_jsds, class_aucs, class_fprs = (np.where(has, v[1:, U + 1], 0.0) for v in (jsd, auc, fdcd))
        if label_map is None:
            label_map = {i + 1: str(i + 1) for i in range(num_classes)}
        iou_range = [f"{i:.2f}" for i in thrs]
        item_size = int(len(iou_range) / 2)
        table_data = [["Classes"] + ["-"] * item_size + ["AUC"] + ["-"] * item_size + ["*"] * item_size + ["JSD"]
                      + ["*"] * item_size + [""] * item_size + [metric] + [""] * item_size,
                      ["IoU Thr."] + iou_range + ["Avg."] + iou_range + ["Avg."] + iou_range + ["Avg."]]

        def row(name, a, j, f):
            return [name] + list(np.round(a, 2)) + [np.round(np.mean(a), 2)] + list(np.round(j, 2)) + [np.round(np.mean(j), 2)] \
                + list(np.round(f, 2)) + [np.round(np.mean(f), 2)]

        for i in range(num_classes):
            table_data.append(row(label_map[i + 1], class_aucs[i], class_jsds[i], class_fprs[i]))
        avg_row = []
        for i in range(1, len(table_data[0])):      # (through the string array, as the reference forms it)
            avg_row.append(np.round(np.mean((np.asarray(table_data)[:, i][2:]).astype("float")), 2))
        table_data.append(["Avg. perc"] + avg_row)
        for i in range(U):
            table_data.append(row("Orig. U." + str(i), aucs_orig[i], jsds_orig[i], fprs_orig[i]))
        table_data.append(row("Opt. Combo", aucs_opt, jsds_opt, fprs_opt))
    jsds_orig, aucs_orig, fprs_orig = np.mean(jsds_orig, axis=-1), np.mean(aucs_orig, axis=-1), np.mean(fprs_orig, axis=-1)
    jsds_opt, aucs_opt, fprs_opt = np.mean(jsds_opt, axis=0), np.mean(aucs_opt, axis=0), np.mean(fprs_opt, axis=0)
    with open(_thr_metrics_path(source_path, s, added_name), "w") as file:
        file.write("JSD, AUC, " + metric + " of Each Uncertainty:\n")
        for idx, (j, a, f) in enumerate(zip(jsds_orig, aucs_orig, fprs_orig), start=1):
            file.write(f"Uncertainty {idx}: JSD = {j:.3f}, AUC = {a:.3f}, {metric} = {f:.3f}\n")
        file.write("\nJSD, AUC, " + metric + " of Optimal Uncertainty:\n")
        file.write(f"JSD = {jsds_opt:.3f}, AUC = {aucs_opt:.3f}, {metric} = {fprs_opt:.3f}\n")
    return fprs_opt if opt_params is None else (fprs_opt, table_data)


def collect_thresh_results(opt_uncert, ious, tps_class, eval_iou_thr, params=None, device=0, report=None):
    """`_collect_thresh_results` (:734-749): (correctly_removed, falsely_removed, falsely_remaining, opt_thr) at one IoU
    threshold - boolean masks over the rows, host compares against the threshold the device found; their sums are the device's
    removal counts."""
    s = _settings(params)
    u = np.asarray(opt_uncert, np.float64).reshape(-1)
    ious, tp = np.asarray(ious, np.float64).reshape(-1), np.asarray(tps_class).reshape(-1).astype(bool)
    rep = thr_report(u[None], ious, tp, [float(eval_iou_thr)], s["thr_cd"], s["thr_fpr_tpr"], device=device, report=report)
    opt_thr = rep.thr[0, 0, 0]
    correct = (ious >= float(eval_iou_thr)) & tp
    masks = (u >= opt_thr) & ~correct, (u >= opt_thr) & correct, (u < opt_thr) & ~correct
    counts = (rep.correctly_removed[0, 0, 0], rep.falsely_removed[0, 0, 0], rep.falsely_remaining[0, 0, 0])
    if tuple(int(m.sum()) for m in masks) != tuple(int(c) for c in counts):
        raise RuntimeError("removal counts %s differ from the masks' %s" % (counts, tuple(int(m.sum()) for m in masks)))
    return masks + (opt_thr,)


def clsoptfix_params(all_opt_params, perc_opt_params, all_fdcd, current_fdcd, has_rows=None):
    """The `_clsoptfix` rule (:448-494) as a function: class i keeps its own weights perc_opt_params[i * U : i * U + U] unless
    they do worse on its rows than the global weights - `current_fdcd[i] < all_fdcd[i] or current_fdcd[i] == 100` -, then the
    global weights are put back.  A class without rows (has_rows[i] false) is left alone.  Returns the new list."""
    U = len(all_opt_params)
    fixed = list(perc_opt_params)
    for i in range(len(all_fdcd)):
        if has_rows is not None and not has_rows[i]:
            continue
        if current_fdcd[i] < all_fdcd[i] or current_fdcd[i] == 100:
            fixed[i * U:i * U + U] = list(all_opt_params)
    return fixed


def threshold_analysis(source_path, params, gt_classes, pred_classes, tps_class, ious, selected_uncerts, per_cls=False,
                       label_map=None, device=0, objective=None, report=None, population=DEFAULT_POPULATION,
                       rounds=DEFAULT_ROUNDS, seed=DEFAULT_SEED):
    """The sequence of `MainUncertViz.__init__` (:398-500) on `UncertOptimal(method="population")`: the global weights and their
    report (""), and with per_cls the per-class weights with the `_clsoptpred` and `_clsopt` reports, the `_clsoptfix` rule and
    its report.  The reference's intermediate per-class `_clsoptfix` calls overwrite one file; only the last one is written.
    Returns a dict: all_opt_params, fprs_opt {added_name: value}, tables {added_name: table_data}, and with per_cls
    perc_opt_params, fixed_opt_params, all_fdcd, current_fdcd [C]."""
    gt_classes = np.asarray(gt_classes, np.float64).reshape(-1)
    uncerts = [np.asarray(u, np.float64).reshape(-1) for u in selected_uncerts]
    tps_class, ious = np.asarray(tps_class).reshape(-1).astype(bool), np.asarray(ious, np.float64).reshape(-1)
    search = dict(source_path=source_path, params=params, objective=objective, population=population, rounds=rounds, seed=seed,
                  device=device)
    save = dict(gt_classes=gt_classes, label_map=label_map, device=device, report=report)
    out = {"fprs_opt": {}, "tables": {}}
    all_opt = UncertOptimal(gt_classes, tps_class, ious, uncerts, added_name="", **search).get_optimal_uncertainty()
    out["all_opt_params"] = all_opt
    out["fprs_opt"][""], out["tables"][""] = save_thr_performance(source_path, params, uncerts, _combine(all_opt, uncerts), tps_class,
                                                                ious, opt_params=all_opt, added_name="", **save)
    if not per_cls:
        return out
    perc = UncertOptimal(gt_classes, tps_class, ious, uncerts, added_name="_clsopt", per_cls=True,
                         **search).get_optimal_uncertainty(break_iter=30)
    num_classes, U = int(max(gt_classes)), len(uncerts)
    out["perc_opt_params"] = list(perc)
    out["fprs_opt"]["_clsoptpred"] = save_thr_performance(source_path, params, uncerts,
                                                          combine_per_class(uncerts, pred_classes, perc, num_classes), tps_class,
                                                          ious, added_name="_clsoptpred", **save)
    out["fprs_opt"]["_clsopt"], out["tables"]["_clsopt"] = save_thr_performance(
        source_path, params, uncerts, combine_per_class(uncerts, gt_classes, perc, num_classes), tps_class, ious, opt_params=perc,
        added_name="_clsopt", **save)
    # the rule: per class the global and the class's own weights on that class's rows - two columns, the classes as segments
    s = _settings(params)
    both = np.stack([_combine(all_opt, uncerts), combine_per_class(uncerts, gt_classes, perc, num_classes)])
    rep = thr_report(both, ious, tps_class, s["thr_iou_thrs"], s["thr_cd"], s["thr_fpr_tpr"], gt_classes=gt_classes,
                     device=device, report=report)
    fdcd = rep.fdcd_mean()[1:]
    has_rows = rep.seg_hi[1:] > rep.seg_lo[1:]
    out["all_fdcd"], out["current_fdcd"] = fdcd[:, 0], fdcd[:, 1]
    fixed = clsoptfix_params(all_opt, perc, fdcd[:, 0], fdcd[:, 1], has_rows)
    out["fixed_opt_params"] = fixed
    out["fprs_opt"]["_clsoptfix"], out["tables"]["_clsoptfix"] = save_thr_performance(
        source_path, params, uncerts, combine_per_class(uncerts, gt_classes, fixed, num_classes), tps_class, ious, opt_params=fixed,
        added_name="_clsoptfix", **save)
    return out
