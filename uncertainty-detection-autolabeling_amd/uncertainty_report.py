"""The validation uncertainty report: how good the served and the calibrated box sigma are.

The reference judges a sigma column in two places.  `ValidUncertPlot.__init__` (src/utils_extra.py:378-445, built by
`Validate.launch_val`, validate_model.py:736-794, for every configuration with box uncertainty) appends % missing detections,
misclassification rate, mIoU, RMSE, the decoding method and `ECE Loc aleatoric` / `ECE mcdropout` to model_performance.txt;
`RegressionCalib._conf_all` (src/calibrate_regression.py:231-349) writes one line per calibration method to
regression_logging.txt: share of rows inside +-sigma, ECE, NLL, RMSUE and sharpness.  Both go through `calc_ece`, a Python loop
of 100 levels x N x 4 comparisons (utils_box.py:31-53), once per column and subset.  Here all columns and subsets of a
validation run are ONE device call (C entry point uda_uncert_report_np, csrc/kernels_report.hip; the contract is in
include/uda_hip.h and DESIGN 21) that returns integer tallies and float64 sums; the divisions, roots, roundings and the text stay
on the host, in the reference's statements.

  levels_z                 p_m = np.linspace(0, 1, levels) and z = norm.ppf((1 - p_m) / 2), the reference's levels
  report_np                arrays -> the raw tallies of the device call
  UncertReport             the tallies of B segments x K named columns; `merge`; per segment the numbers of
                           ValidUncertPlot.__init__ (`missing_pct`, `misclassification`, `miou`, `rmse`, `ece`) and per column
                           those of _conf_all (`coverage_pct`, `ece`, `nll`, `rmsue`, `sharpness`) and `ece_per_coordinate`
  report / per_class       -> UncertReport of all rows as one segment / of one segment per class
  relative_ece             `_relative_calc_ece` (calibrate_regression.py:46-61) through the same call
  model_performance_lines  the lines ValidUncertPlot.__init__ appends to model_performance.txt
  regression_logging_lines the two lines _conf_all appends to regression_logging.txt
  from_filtered            the report of what `writers.validate_to_file` returns

What differs from the reference, on purpose: `calc_nll` turns sigma = 0 into +-1.8e308 through nan_to_num, an overflow artefact -
here an element whose sigma is 0 or not finite is left out of the NLL (sum and divisor) and counted (`n_degenerate`); the
reference squares in float32 for the sharpness and takes the RMSE as a TensorFlow reduction of unpinned order - here both are
float64 sums of a stated order, the sharpness rounded to float32 at the end.

Not built: the plots, the uncertainty_toolbox metrics block (`uct.metrics.get_all_metrics`), the PIT / CDF scatter of `_cdf` and
the fitting of calibrators.  The classification reliability bins (`_calibr_bins`) are `class_report`.
"""
import numpy as np

from . import capi

ROWS, MAX_K, MAX_L, MAX_B, MAX_ROWS = capi.REPORT_ROWS, capi.REPORT_MAX_K, capi.REPORT_MAX_L, capi.REPORT_MAX_B, capi.REPORT_MAX_ROWS
SEG_COUNTS = ("n_rows", "n_iou_zero", "n_misclassified", "n_gt_nonzero")
COL_COUNTS = ("covered_all", "n_res_nonzero", "n_degenerate")
SEG_SUMS = ("S_iou", "S_sqerr")
COL_SUMS = ("S_sigma2", "S_ue", "S_nll")
KINDS = {"aleatoric": "albox", "mcdropout": "mcbox"}      # the folder ValidUncertPlot saves under -> the sigma column it is given


def levels_z(levels=100):
    """-> p_m, z of calc_ece (utils_box.py:39-45).  For 100 levels z[0] = 0.0 and z[99] = -inf."""
    from scipy import stats
    p_m = np.linspace(0, 1, int(levels))
    return p_m, stats.norm.ppf((1 - p_m) / 2)


def _inputs(gt, pred, sigmas, gt_classes, classes, segments):
    gt = np.ascontiguousarray(np.asarray(gt, np.float64).reshape(-1, 4))
    pred = np.ascontiguousarray(np.asarray(pred, np.float64).reshape(-1, 4))
    N = len(gt)
    if len(pred) != N:
        raise ValueError("uncertainty report: %d ground-truth rows, %d predicted" % (N, len(pred)))
    sig = [np.asarray(s, np.float64) for s in sigmas]
    for k, s in enumerate(sig):
        if s.shape != (N, 4):
            raise ValueError("uncertainty report: sigma column %d has shape %s, not (%d, 4)" % (k, s.shape, N))
    if not 1 <= len(sig) <= MAX_K:
        raise ValueError("uncertainty report: %d sigma columns in one call, 1..%d are taken" % (len(sig), MAX_K))
    sig = np.ascontiguousarray(np.stack(sig))
    gc = np.ascontiguousarray(np.asarray(gt_classes, np.float64).reshape(-1))
    pc = np.ascontiguousarray(np.asarray(classes, np.float64).reshape(-1))
    if len(gc) != N or len(pc) != N:
        raise ValueError("uncertainty report: %d rows, %d ground-truth classes, %d classes" % (N, len(gc), len(pc)))
    off = np.ascontiguousarray(np.asarray([0, N] if segments is None else segments, np.int64).reshape(-1))
    if len(off) < 2 or off[0] != 0 or off[-1] != N or (np.diff(off) < 0).any():
        raise ValueError("uncertainty report: segments must ascend from 0 to the %d rows" % N)
    if len(off) - 1 > MAX_B or N > MAX_ROWS:
        raise ValueError("uncertainty report: %d segments and %d rows, at most %d and %d" % (len(off) - 1, N, MAX_B, MAX_ROWS))
    return gt, pred, sig, gc, pc, off


def report_np(gt, pred, sigmas, gt_classes, classes, segments=None, levels=100, device=0):
    """gt / pred [N, 4], sigmas: K arrays [N, 4], gt_classes / classes [N]; segments: offsets [B + 1] ascending from 0 to N (None:
    all rows are one segment) -> the dict of the arrays of uda_uncert_report_np - seg_counts [B, 4], col_counts [B, K, 3],
    ece_count [B, K, 4, L], seg_sums [B, 2], col_sums [B, K, 3] - with off, p_m and z."""
    gt, pred, sig, gc, pc, off = _inputs(gt, pred, sigmas, gt_classes, classes, segments)
    p_m, z = levels_z(levels)
    if not 1 <= len(z) <= MAX_L:
        raise ValueError("uncertainty report: %d levels, 1..%d are taken" % (len(z), MAX_L))
    z = np.ascontiguousarray(z, np.float64)
    B, K, L = len(off) - 1, len(sig), len(z)
    res = dict(seg_counts=np.zeros((B, 4), np.int64), col_counts=np.zeros((B, K, 3), np.int64), ece_count=np.zeros((B, K, 4, L), np.int64),
               seg_sums=np.zeros((B, 2), np.float64), col_sums=np.zeros((B, K, 3), np.float64))
    lib = capi.load()
    rc = lib.uda_uncert_report_np(int(device), B, K, L, off.ctypes.data, gt.ctypes.data, pred.ctypes.data, gc.ctypes.data, pc.ctypes.data,
                                  sig.ctypes.data, z.ctypes.data, res["seg_counts"].ctypes.data, res["col_counts"].ctypes.data,
                                  res["ece_count"].ctypes.data, res["seg_sums"].ctypes.data, res["col_sums"].ctypes.data)
    capi.check(lib, None, rc, "uda_uncert_report_np")
    res.update(off=off, p_m=p_m, z=z)
    return res


def _ratio(num, den):
    return num / den if den else float("nan")


class UncertReport:
    """The tallies of B segments x K sigma columns.  `names`: the columns' names, `labels`: the segments' (class ids for
    `per_class`, None for one segment of all rows).  Every number takes `segment` (index, default 0) and, where it belongs to a
    column, `column` (name or index, default 0).  A number of an empty segment is nan."""

    def __init__(self, res, names=None, labels=None):
        self.seg_counts, self.col_counts, self.ece_count = (np.array(res[k], np.int64) for k in ("seg_counts", "col_counts", "ece_count"))
        self.seg_sums, self.col_sums = np.array(res["seg_sums"], np.float64), np.array(res["col_sums"], np.float64)
        self.p_m = np.array(res["p_m"], np.float64)
        K = self.col_counts.shape[1]
        self.names = [str(n) for n in names] if names is not None else [str(k) for k in range(K)]
        self.labels = list(labels) if labels is not None else None
        if len(self.names) != K or len(self.p_m) != self.ece_count.shape[3]:
            raise ValueError("uncertainty report: %d names for %d columns, %d levels for %d counts" %
                             (len(self.names), K, len(self.p_m), self.ece_count.shape[3]))

    def __len__(self):
        return len(self.seg_counts)

    def merge(self, other):
        """Adds the tallies of `other` (same columns, segments and levels), as a validation run in parts needs.  Counts add
        exactly, so % missing, misclassification, coverage and every ECE of the merged report are those of one call over all
        rows.  A float64 sum becomes `self + other`, one more node above the two trees: that is the whole's tree bit for bit when
        `self` holds a power of two of rows that is no less than `other`'s count, and within the summation bound otherwise."""
        if self.names != other.names or self.labels != other.labels or not np.array_equal(self.p_m, other.p_m):
            raise ValueError("uncertainty report: merge needs the same columns, segments and levels")
        for k in ("seg_counts", "col_counts", "ece_count", "seg_sums", "col_sums"):
            setattr(self, k, getattr(self, k) + getattr(other, k))
        return self

    def column(self, column):
        return column if isinstance(column, (int, np.integer)) else self.names.index(column)

    def count(self, name, segment=0, column=0):
        if name in SEG_COUNTS:
            return int(self.seg_counts[segment, SEG_COUNTS.index(name)])
        return int(self.col_counts[segment, self.column(column), COL_COUNTS.index(name)])

    def total(self, name, segment=0, column=0):
        if name in SEG_SUMS:
            return self.seg_sums[segment, SEG_SUMS.index(name)]
        return self.col_sums[segment, self.column(column), COL_SUMS.index(name)]

    # ---- ValidUncertPlot.__init__ (utils_extra.py:417-422)
    def missing_pct(self, segment=0):
        return _ratio(self.count("n_iou_zero", segment), self.count("n_rows", segment)) * 100

    def misclassification(self, segment=0):
        return _ratio(self.count("n_misclassified", segment), self.count("n_rows", segment))

    def miou(self, segment=0):
        return _ratio(self.total("S_iou", segment), self.count("n_rows", segment))

    def rmse(self, segment=0):
        return float(np.sqrt(_ratio(self.total("S_sqerr", segment), self.count("n_gt_nonzero", segment))))

    def ece(self, column=0, segment=0):
        """calc_ece of the flattened arrays (:422; _conf_all:277-283): the four coordinates counted together."""
        n = 4 * self.count("n_rows", segment)
        if n == 0:
            return np.float64("nan")
        counts = self.ece_count[segment, self.column(column)].sum(axis=0)
        emp_conf = [c / n for c in counts]
        return np.mean(np.abs(emp_conf - self.p_m))

    def ece_per_coordinate(self, column=0, segment=0):
        """calc_ece of one coordinate's column at a time -> [4]."""
        n = self.count("n_rows", segment)
        if n == 0:
            return np.full(4, np.nan)
        return np.array([np.mean(np.abs([c / n for c in self.ece_count[segment, self.column(column), co]] - self.p_m)) for co in range(4)])

    def ece_box(self, column=0, segment=0):
        """calc_ece of the [N, 4] arrays (utils_box.py:51-52): the mean over levels and coordinates."""
        n = self.count("n_rows", segment)
        if n == 0:
            return np.float64("nan")
        counts = self.ece_count[segment, self.column(column)]                 # [4, L]
        emp_conf = [counts[:, i] / n for i in range(counts.shape[1])]
        return np.mean(np.abs(emp_conf - np.swapaxes([self.p_m] * 4, 0, 1)))

    # ---- RegressionCalib._conf_all (calibrate_regression.py:258-333), before its rounding
    def coverage_pct(self, column=0, segment=0):
        return _ratio(self.count("covered_all", segment, column), self.count("n_rows", segment)) * 100

    def nll(self, column=0, segment=0):
        n = 4 * self.count("n_rows", segment) - self.count("n_degenerate", segment, column)
        return _ratio(self.total("S_nll", segment, column), n)

    def rmsue(self, column=0, segment=0):
        return np.sqrt(_ratio(self.total("S_ue", segment, column), self.count("n_res_nonzero", segment, column)))

    def sharpness(self, column=0, segment=0):
        return np.float32(np.sqrt(_ratio(self.total("S_sigma2", segment, column), 4 * self.count("n_rows", segment))))


def _named(sigmas):
    if isinstance(sigmas, dict):
        return list(sigmas), list(sigmas.values())
    sigmas = list(sigmas)
    return None, sigmas


def report(gt, pred, sigmas, gt_classes, classes, levels=100, device=0, engine=None):
    """All rows as one segment -> UncertReport.  sigmas: a dict name -> [N, 4] or a sequence of [N, 4]; engine: what computes the
    tallies (default `report_np`, the device)."""
    names, cols = _named(sigmas)
    return UncertReport((engine or report_np)(gt, pred, cols, gt_classes, classes, None, levels, device), names)


def per_class(gt, pred, sigmas, gt_classes, classes, class_ids, levels=100, device=0, engine=None):
    """One segment per entry of `class_ids`, holding the rows whose GROUND-TRUTH class is that id in their given order (a stable
    sort); rows of other classes are left out, a class without rows gives an empty segment -> UncertReport with labels."""
    names, cols = _named(sigmas)
    gc = np.asarray(gt_classes).reshape(-1)
    picks = [np.where(gc == c)[0] for c in class_ids]
    order = np.concatenate(picks) if picks else np.zeros(0, np.int64)
    off = np.concatenate([[0], np.cumsum([len(p) for p in picks])]).astype(np.int64)
    take = lambda a: np.asarray(a)[order]                                    # noqa: E731
    res = (engine or report_np)(take(gt), take(pred), [take(s) for s in cols], take(gt_classes), take(classes), off, levels, device)
    return UncertReport(res, names, labels=list(class_ids))


def relative_ece(norm_residuals, norm_sigmas, levels=100, device=0, engine=None):
    """`_relative_calc_ece` (calibrate_regression.py:46-61) of relativised residuals [N, 4] (or [N] for one coordinate) against
    every relativised sigma of `norm_sigmas` (dict or sequence, same shape): the residuals go in as `pred` against gt = 0, so the
    level test is the reference's `norm_residuals <= |sigma * z|`.  Residuals are absolute values; a negative one is refused (the
    reference would count it at every level).  -> one ECE per column, the [N, 4] form's mean or the one coordinate's."""
    names, cols = _named(norm_sigmas)
    r = np.asarray(norm_residuals, np.float64)
    one = r.ndim == 1
    if (r < 0).any():
        raise ValueError("relative_ece: residuals are absolute values, got a negative one")
    if one:                                                                    # one coordinate: pad the other three, read the first
        r = np.stack([r, np.zeros_like(r), np.zeros_like(r), np.zeros_like(r)], 1)
        cols = [np.stack([np.asarray(s, np.float64)] + [np.ones(len(r))] * 3, 1) for s in cols]
    zeros = np.zeros(len(r))
    rep = UncertReport((engine or report_np)(np.zeros_like(r), r, cols, zeros, zeros, None, levels, device), names)
    out = [rep.ece_per_coordinate(k)[0] if one else rep.ece_box(k) for k in range(len(cols))]
    return dict(zip(names, out)) if names is not None else out


# ---------------------------------------------------------------------------------- text
def model_performance_lines(report, which, decoding, exists=False, column=None, segment=0):
    """What ValidUncertPlot.__init__ appends to model_performance.txt (utils_extra.py:423-445) for the kind `which` ("aleatoric"
    / "mcdropout", the last part of its save path; its sigma column is `column`, default KINDS[which]): six lines, or - where the
    file `exists` already, as it does for the second kind - the ECE line alone."""
    ece = report.ece(KINDS.get(which, which) if column is None else column, segment)
    if exists:
        return ["ECE " + which + ": " + str(ece) + " \n"]
    return ["% Missing Detections: " + str(report.missing_pct(segment)) + " \n",
            "Misclassification rate: " + str(report.misclassification(segment)) + " \n",
            "mIoU: " + str(report.miou(segment)) + " \n", "RMSE: " + str(report.rmse(segment)) + " \n",
            "Uncertainty Decoding: " + decoding + " \n", "ECE Loc " + which + ": " + str(ece) + " \n"]


def regression_logging_lines(report, method, calibrated, column=0, segment=0):
    """The two lines _conf_all appends to regression_logging.txt (calibrate_regression.py:269-349) for sigma column `column`:
    `calibrated` selects the wording, `method` names the calibration in it."""
    pct = str(round(report.coverage_pct(column, segment), 1))
    word = "Calibrated" if calibrated else "Uncalibrated"
    head = "% of true values in interval ± σ of predicted values for all coordinates"
    head += (" after calibration with " + method + ": ") if calibrated else ": "
    return [head + pct + " \n",
            word + " ECE " + str(np.round(report.ece(column, segment), 4)) + ", " + word + " NLL " + str(np.round(report.nll(column, segment), 4)) +
            ", " + word + " RMSUE " + str(np.round(report.rmsue(column, segment), 4)) + ", " + word + " Sharp. " +
            str(np.round(report.sharpness(column, segment), 4)) + " \n"]


def from_filtered(filtered, calibrated=True, levels=100, device=0, engine=None):
    """The report of the matched rows `writers.validate_to_file` returns: columns "albox" / "mcbox" where the model serves them,
    then - with `calibrated` - every calibrated variant in filtered["calibrated"] ("<method>_albox", ...).  One segment of all
    rows; the float32 columns go in as the float64 of the same value."""
    sig = {k: filtered[k] for k in ("albox", "mcbox") if filtered.get(k) is not None}
    if calibrated:
        sig.update({k: v for k, v in (filtered.get("calibrated") or {}).items() if k.endswith(("_albox", "_mcbox")) and np.ndim(v) == 2})
    if not sig:
        raise ValueError("uncertainty report: the model serves no box uncertainty (no albox, no mcbox)")
    return report(filtered["gt_boxes"], filtered["boxes"], sig, filtered["gt_classes"], filtered["classes"], levels, device, engine)
