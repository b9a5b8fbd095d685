"""The classification calibration report: whether the served and the calibrated class probabilities are calibrated.

The reference answers that in `ClassificationCalib` (src/calibrate_classification.py): `_calibr_plot` (:250-440) runs once per
configuration - uncalibrated, TS all, TS per class, isotonic all, isotonic per class - and calls `_calibr_bins` (:97-143) once
per class and once over the arg-max class: one `np.digitize` / `np.bincount` pass over the validation rows per (configuration,
target), from which the reliability diagram, ECE, MCE and - with the Brier score, the NLL and the SCE - the plot titles follow.
Here every (segment, configuration, target) of a validation run is ONE device call (C entry point uda_class_report_np,
csrc/kernels_classrep.hip; the contract is in include/uda_hip.h and DESIGN 22) that returns integer tallies and float64 sums; the
divisions, the selection of the non-empty bins, the roundings and the text stay on the host, in the reference's statements.

  uniform_edges / quantile_edges   the two bin definitions of `_calibr_bins` (:115-122)
  report_np                        arrays -> the raw tallies of the device call
  ClassReport                      the tallies of B segments x M named tables x (C + 1) targets; `merge`; per (table, target,
                                   segment) `bins` (the reference's freq, prob, bin_prob, bin_count), `ece`, `mce`, `brier`, and
                                   per (table, segment) `brier_all`, `nll`, `sce`
  report                           -> ClassReport
  tables_from_logits               the five probability tables of `_calibr_plot` from logits and the calibrators' models
  title_lines                      the two plot titles (:371-378, 407-419) as text
  from_filtered                    the report of what `calibration.gather_detections` or `writers.validate_to_file` returns, on
                                   the reference's evaluation split (rows int(0.8 n) onwards)

What differs from the reference, on purpose.  A bin's sum of probabilities is a float64 tree sum of a stated order where
`np.bincount` keeps a running sum: `prob`, ECE, MCE and the Brier score agree within the summation bound, counts, hits, the
selection of the non-empty bins and `bin_prob` exactly.  A value at or above the last edge (or a NaN) makes the reference raise an
IndexError; the device counts it in a slot of its own and `bins` raises that error by default, or folds the slot into the last bin
with overflow="last".  The NLL is Keras's CategoricalCrossentropy() row term on probabilities in float64 (TensorFlow would use the
tensors' dtype); the reference's UNCALIBRATED `self.nll` feeds logits to that loss, which expects probabilities - that is not
reproduced, the uncalibrated table's NLL here is that of its softmax probabilities.

Not built: the plots themselves and the fitting of the calibrators (the caller supplies temperatures and isotonic tables, as for
`calibration.ClassCalibrator`).
"""
import numpy as np

from . import capi
from .calibration import IsoTable

ROWS, MAX_B, MAX_M, MAX_C, MAX_E, MAX_ROWS = (capi.CLASSREP_ROWS, capi.CLASSREP_MAX_B, capi.CLASSREP_MAX_M, capi.CLASSREP_MAX_C,
                                              capi.CLASSREP_MAX_E, capi.CLASSREP_MAX_ROWS)
METHOD_NAMES = {"uncalibrated": "", "ts_all": "all_calib_TS", "ts_percls": "perclass_calib_TS", "iso_all": "all_calib_IR",
                "iso_percls": "perclass_calib_IR"}     # the model's key -> `calib_methd` of _calibr_plot (:294-321)


# ---------------------------------------------------------------------------------- bin edges (:115-122)
def uniform_edges(n_bins=10):
    """`np.linspace(0.0, 1.0 + 1e-8, n_bins + 1)` (:122)."""
    return np.linspace(0.0, 1.0 + 1e-8, int(n_bins) + 1)


def argmax_rows(p):
    """[n, C] -> `p.argmax(axis=-1)`: the first NaN of a row if it holds one, else its first maximum."""
    return np.asarray(p).argmax(axis=-1)


def _quantile_row(ypred, n_bins):
    if len(ypred) == 0:                                      # (np.quantile of nothing raises; an empty segment bins nothing)
        return uniform_edges(n_bins)
    b = np.linspace(0.0, 1.0 + 1e-8, n_bins + 1)
    b[-1] -= 1e-8
    bins = np.quantile(ypred, b)
    bins = np.unique(bins).astype(np.float64)
    bins[-1] = 1 + 1e-8
    if len(bins) == 1:                                       # all values equal: the call takes two edges at least (see quantile_edges)
        bins = np.array([-np.inf, bins[0]])
    return bins


def quantile_edges(prob, segments=None, n_bins=10):
    """The quantile strategy of `_calibr_bins` (:115-120) on the host.  prob [n]: one target's ypred -> its edges.  prob [M, N, C]
    (with `segments`, default one of all rows): -> the list of B * M * (C + 1) edge rows `report_np` takes, row
    (b * M + m) * (C + 1) + t for target t of table m of segment b, target C binning the arg-max probability.  Where all values
    of a target are equal the reference is left with ONE edge; the device call takes two at least, so -inf is put in front: bin 0
    is then empty and drops out of the non-empty selection, which leaves the reference's arrays.  An empty segment gets the
    uniform edges (it bins nothing)."""
    prob = np.asarray(prob, np.float64)
    if prob.ndim == 1:
        return _quantile_row(prob, int(n_bins))
    M, N, C = prob.shape
    off = np.asarray([0, N] if segments is None else segments, np.int64).reshape(-1)
    rows = []
    for b in range(len(off) - 1):
        for m in range(M):
            p = prob[m, off[b]:off[b + 1]]
            rows += [_quantile_row(p[:, t], int(n_bins)) for t in range(C)]
            rows.append(_quantile_row(p[np.arange(len(p)), argmax_rows(p)] if len(p) else p[:, 0], int(n_bins)))
    return rows


# ---------------------------------------------------------------------------------- the device call
def _inputs(prob, label, segments, edges):
    prob = np.asarray(prob, np.float64)
    if prob.ndim == 2:
        prob = prob[None]
    if prob.ndim != 3:
        raise ValueError("class report: prob has shape %s, not (M, N, C)" % (prob.shape,))
    prob = np.ascontiguousarray(prob)
    M, N, C = prob.shape
    lab = np.asarray(label).reshape(-1)
    if len(lab) != N:
        raise ValueError("class report: %d rows, %d labels" % (N, len(lab)))
    if N and not (np.asarray(lab, np.float64) == np.floor(np.asarray(lab, np.float64))).all():
        raise ValueError("class report: a label is not a whole number")
    lab = np.ascontiguousarray(lab, np.int32)
    if not (1 <= M <= MAX_M and 1 <= C <= MAX_C):
        raise ValueError("class report: %d tables of %d classes, 1..%d and 1..%d are taken" % (M, C, MAX_M, MAX_C))
    if N and (lab.min() < 0 or lab.max() >= C):
        raise ValueError("class report: a label is outside 0..%d" % (C - 1))
    off = np.ascontiguousarray(np.asarray([0, N] if segments is None else segments, np.int64).reshape(-1))
    if len(off) < 2 or off[0] != 0 or off[-1] != N or (np.diff(off) < 0).any():
        raise ValueError("class report: segments must ascend from 0 to the %d rows" % N)
    B = len(off) - 1
    if B > MAX_B or N > MAX_ROWS:
        raise ValueError("class report: %d segments and %d rows, at most %d and %d" % (B, N, MAX_B, MAX_ROWS))
    if edges is None:
        rows = [uniform_edges()]
    elif np.ndim(edges[0]) == 0:
        rows = [np.asarray(edges, np.float64)]
    else:
        rows = [np.asarray(e, np.float64).reshape(-1) for e in edges]
    G = len(rows)
    if G not in (1, B * M * (C + 1)):
        raise ValueError("class report: %d edge rows, 1 or B * M * (C + 1) = %d are taken" % (G, B * M * (C + 1)))
    ne = np.ascontiguousarray([len(r) for r in rows], np.int32)
    if ne.min() < 2 or ne.max() > MAX_E:
        raise ValueError("class report: an edge row holds %d edges, 2..%d are taken" % (ne.min() if ne.min() < 2 else ne.max(), MAX_E))
    ed = np.zeros((G, int(ne.max())), np.float64)
    for g, r in enumerate(rows):
        ed[g, :len(r)] = r
        if not (r[:-1] < r[1:]).all():
            raise ValueError("class report: the edges of row %d do not ascend strictly (or hold a NaN)" % g)
    return prob, lab, off, ed, ne


def report_np(prob, label, segments=None, edges=None, device=0):
    """prob [M, N, C] (or [N, C] for one table), label [N] (the true class index); segments: offsets [B + 1] ascending from 0 to N
    (None: all rows are one segment); edges: None (the uniform edges of 10 bins), one row of ascending edges shared by all
    targets, or B * M * (C + 1) rows (see `quantile_edges`) -> the dict of the arrays of uda_class_report_np - bin_count / bin_hits
    / bin_sum [B, M, C + 1, E + 1], brier_sum [B, M, C], nll_sum [B, M], tab_counts [B, M, 2] - with off, edges [G, E], n_edges [G]."""
    prob, lab, off, ed, ne = _inputs(prob, label, segments, edges)
    M, N, C = prob.shape
    B, (G, E) = len(off) - 1, ed.shape
    res = dict(bin_count=np.zeros((B, M, C + 1, E + 1), np.int64), bin_hits=np.zeros((B, M, C + 1, E + 1), np.int64),
               bin_sum=np.zeros((B, M, C + 1, E + 1), np.float64), brier_sum=np.zeros((B, M, C), np.float64),
               nll_sum=np.zeros((B, M), np.float64), tab_counts=np.zeros((B, M, 2), np.int64))
    lib = capi.load()
    rc = lib.uda_class_report_np(int(device), B, M, C, G, E, off.ctypes.data, prob.ctypes.data, lab.ctypes.data, ed.ctypes.data,
                                 ne.ctypes.data, res["bin_count"].ctypes.data, res["bin_hits"].ctypes.data, res["bin_sum"].ctypes.data,
                                 res["brier_sum"].ctypes.data, res["nll_sum"].ctypes.data, res["tab_counts"].ctypes.data)
    capi.check(lib, None, rc, "uda_class_report_np")
    res.update(off=off, edges=ed, n_edges=ne)
    return res


class ClassReport:
    """The tallies of B segments x M probability tables x (C + 1) targets.  `names`: the tables' names (the reference's
    `calib_methd`: "" is the uncalibrated table), `labels`: the segments'.  Every number takes `table` (name or index, default 0),
    `target` (a class index, or "all" / C for the arg-max target; default "all") and `segment` (index, default 0).  A number of
    an empty segment is nan.  `overflow`: what `bins` and the numbers built on it do when the slot past the last edge is
    populated - "raise" (default; the reference's IndexError) or "last" (fold it into the last bin)."""

    INT_KEYS, SUM_KEYS = ("bin_count", "bin_hits", "tab_counts"), ("bin_sum", "brier_sum", "nll_sum")

    def __init__(self, res, names=None, labels=None, overflow="raise"):
        for k in self.INT_KEYS:
            setattr(self, k, np.array(res[k], np.int64))
        for k in self.SUM_KEYS:
            setattr(self, k, np.array(res[k], np.float64))
        self.off = np.array(res["off"], np.int64)
        self.n_rows = np.diff(self.off)
        self.edges, self.n_edges = np.array(res["edges"], np.float64), np.array(res["n_edges"], np.int64)
        B, M, T, _ = self.bin_count.shape
        self.C = T - 1
        self.names = [str(n) for n in names] if names is not None else [str(m) for m in range(M)]
        self.labels = list(labels) if labels is not None else None
        if overflow not in ("raise", "last"):
            raise ValueError("class report: overflow is 'raise' or 'last'")
        self.overflow = overflow
        if len(self.names) != M or len(self.n_rows) != B or len(self.n_edges) not in (1, B * M * T):
            raise ValueError("class report: %d names for %d tables, %d segments for %d, %d edge rows" %
                             (len(self.names), M, len(self.n_rows), B, len(self.n_edges)))

    def __len__(self):
        return len(self.n_rows)

    def merge(self, other):
        """Adds the tallies of `other` (same tables, segments and edges), as a validation run in parts needs.  Counts and hits add
        exactly, so `freq`, `bin_count`, `bin_prob` and the selection of the non-empty bins of the merged report are those of one
        call over all rows.  A float64 sum becomes `self + other`, one more node above the two trees: that is the whole's tree bit
        for bit when `self` holds a power of two of rows that is no less than `other`'s count, and within the summation bound
        otherwise."""
        if (self.names != other.names or self.labels != other.labels or not np.array_equal(self.n_edges, other.n_edges) or
                not np.array_equal(self.edges, other.edges)):
            raise ValueError("class report: merge needs the same tables, segments and edges")
        for k in self.INT_KEYS + self.SUM_KEYS + ("n_rows",):
            setattr(self, k, getattr(self, k) + getattr(other, k))
        self.off = np.concatenate([[0], np.cumsum(self.n_rows)]).astype(np.int64)
        return self

    def table(self, table):
        return table if isinstance(table, (int, np.integer)) else self.names.index(table)

    def target(self, target):
        return self.C if isinstance(target, str) and target == "all" else int(target)

    def target_edges(self, table=0, target="all", segment=0):
        """The edges target `target` of (table, segment) was binned with."""
        m, t = self.table(table), self.target(target)
        g = 0 if len(self.n_edges) == 1 else (segment * len(self.names) + m) * (self.C + 1) + t
        return self.edges[g, :self.n_edges[g]]

    def overflow_count(self, table=0, target="all", segment=0):
        """The rows at or above the last edge, NaN included: what makes the reference raise."""
        m, t = self.table(table), self.target(target)
        return int(self.bin_count[segment, m, t, len(self.target_edges(m, t, segment))])

    def _tallies(self, table, target, segment, overflow):
        m, t = self.table(table), self.target(target)
        bins = self.target_edges(m, t, segment)
        ne = len(bins)
        total, hits, sums = (a[segment, m, t, :ne + 1].copy() for a in (self.bin_count, self.bin_hits, self.bin_sum))
        if total[ne]:
            if (overflow or self.overflow) != "last":
                raise IndexError("class report: %d rows of table %r, target %r, segment %d lie at or above the last edge %r (or are "
                                 "NaN): boolean index did not match, as the reference's `bins[nonzero]` says; overflow='last' folds "
                                 "them into the last bin" % (total[ne], self.names[m], target, segment, bins[-1]))
            total[ne - 1] += total[ne]
            hits[ne - 1] += hits[ne]
            sums[ne - 1] = sums[ne - 1] + sums[ne]
        return bins, total[:ne], hits[:ne], sums[:ne]

    def bins(self, table=0, target="all", segment=0, overflow=None):
        """`_calibr_bins` (:124-139) -> dict freq, prob, bin_prob, bin_count over the non-empty bins."""
        bins, bin_total, bin_true, bin_sums = self._tallies(table, target, segment, overflow)
        nonzero = bin_total != 0
        prob_true = bin_true[nonzero] / bin_total[nonzero]
        prob_pred = bin_sums[nonzero] / bin_total[nonzero]
        return dict(freq=prob_true, prob=prob_pred, bin_prob=np.insert(bins[nonzero], 0, 0), bin_count=bin_total[nonzero])

    def ece(self, table=0, target="all", segment=0, overflow=None):
        """:140-142 (the ACE under the quantile edges)."""
        n = int(self.n_rows[segment])
        if n == 0:
            return np.float64("nan")
        b = self.bins(table, target, segment, overflow)
        return np.sum(np.abs(b["freq"] - b["prob"]) * (b["bin_count"] / n))

    def mce(self, table=0, target="all", segment=0, overflow=None):
        """:143."""
        if int(self.n_rows[segment]) == 0:
            return np.float64("nan")
        b = self.bins(table, target, segment, overflow)
        return np.max(np.abs(b["freq"] - b["prob"]))

    def brier(self, table=0, target=0, segment=0):
        """`np.mean((y_pred[:, target] - y_true[:, target]) ** 2)` (:370) of a class."""
        n = int(self.n_rows[segment])
        return self.brier_sum[segment, self.table(table), self.target(target)] / n if n else np.float64("nan")

    def brier_all(self, table=0, segment=0):
        """`np.mean((y_pred - y_true) ** 2)` (:391) over rows and classes."""
        n = int(self.n_rows[segment])
        return np.sum(self.brier_sum[segment, self.table(table)]) / (n * self.C) if n else np.float64("nan")

    def nll(self, table=0, segment=0):
        """The mean of Keras's CategoricalCrossentropy() row terms (:324-326) over the rows that have one (see `count`)."""
        m = self.table(table)
        n = int(self.n_rows[segment]) - int(self.tab_counts[segment, m, 1])
        return self.nll_sum[segment, m] / n if n else np.float64("nan")

    def count(self, name, table=0, segment=0):
        """"clipped": the rows whose probability of the true class was clipped to [1e-7, 1 - 1e-7]; "left_out": the rows without
        an NLL term (a non-finite entry, or a row sum of 0)."""
        return int(self.tab_counts[segment, self.table(table), ("clipped", "left_out").index(name)])

    def sce(self, table=0, segment=0, overflow=None):
        """`np.mean(eces)` of the per-class `np.around(ece, 3)` (:361, 413)."""
        return np.mean([np.around(self.ece(table, t, segment, overflow), 3) for t in range(self.C)])


def report(prob, label, names=None, segments=None, edges=None, labels=None, device=0, engine=None, overflow="raise"):
    """-> ClassReport of the M tables `prob` [M, N, C] (or a dict name -> [N, C]).  engine: what computes the tallies (default
    `report_np`, the device)."""
    if isinstance(prob, dict):
        names, prob = list(prob), np.stack([np.asarray(v, np.float64) for v in prob.values()])
    return ClassReport((engine or report_np)(prob, label, segments, edges, device), names, labels, overflow)


# ---------------------------------------------------------------------------------- the five tables of _calibr_plot
def stable_softmax(logits):
    """`stable_softmax` (utils_class.py:36-41), all rows at once: exp(x - max(x)) / sum(exp(x - max(x))) in the logits' dtype."""
    x = np.asarray(logits)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / np.sum(e, axis=-1, keepdims=True)


def iso_predict(table, x):
    """`IsotonicRegression(out_of_bounds="clip").predict` from the thresholds table: clip to the fitted range, interpolate
    linearly in float64, cast to the input's dtype."""
    x = np.asarray(x)
    t = np.clip(x.astype(np.float64), table.x[0], table.x[-1])
    if table.x.size == 1:
        return np.full(x.shape, table.y[0]).astype(x.dtype)
    return np.interp(t, table.x, table.y).astype(x.dtype)


def _renormalise(ycalibs, C):
    return ycalibs / np.stack([np.sum(ycalibs, axis=-1)] * C, axis=-1)      # (:304-306, 316-318)


def tables_from_logits(logits, ts_all=None, ts_percls=None, iso_all=None, iso_percls=None):
    """The probability tables `_calibr_plot` bins (:284-320), from logits [N, C] and the models a `ClassCalibrator` takes:
    uncalibrated `stable_softmax(logits)`; ts_all / ts_percls `stable_softmax(logits / temperature)`; iso_all the one table's
    prediction of the flattened softmax, iso_percls class c's table on column c, either divided by its row sum.  The arithmetic is
    numpy's on what is given (float32 logits with float32 temperatures stay float32, as in the reference); the tables come back
    as float64 of those values.  -> (tables [M, N, C] float64, names): the uncalibrated table first, then the models given, named
    with the reference's `calib_methd` ("" / all_calib_TS / perclass_calib_TS / all_calib_IR / perclass_calib_IR)."""
    logits = np.asarray(logits)
    if logits.ndim != 2:
        raise ValueError("class report: logits have shape %s, not (N, C)" % (logits.shape,))
    C = logits.shape[1]
    soft = stable_softmax(logits)
    tables, names = [soft], [METHOD_NAMES["uncalibrated"]]
    if ts_all is not None:
        tables.append(stable_softmax(logits / ts_all))
        names.append(METHOD_NAMES["ts_all"])
    if ts_percls is not None:
        t = np.asarray(ts_percls)
        if t.shape != (C,):
            raise ValueError("class report: ts_percls needs %d temperatures" % C)
        tables.append(stable_softmax(logits / t))
        names.append(METHOD_NAMES["ts_percls"])
    if iso_all is not None:
        if not isinstance(iso_all, IsoTable):
            raise ValueError("class report: iso_all is one IsoTable")
        tables.append(_renormalise(iso_predict(iso_all, soft.flatten()).reshape(soft.shape), C))
        names.append(METHOD_NAMES["iso_all"])
    if iso_percls is not None:
        iso_percls = list(iso_percls)
        if len(iso_percls) != C:
            raise ValueError("class report: iso_percls needs %d IsoTables" % C)
        tables.append(_renormalise(np.stack([iso_predict(iso_percls[i], soft[:, i]) for i in range(C)], axis=1), C))
        names.append(METHOD_NAMES["iso_percls"])
    return np.stack([np.asarray(t, np.float64) for t in tables]), names


# ---------------------------------------------------------------------------------- text
def title_lines(report, table=0, target="all", segment=0, quantile=False, overflow=None):
    """The plot title `_calibr_plot` sets: for a class (:371-378) "ECE x\\nMCE y     Brier: z", for the arg-max target "all"
    (:407-419) "ECE x     NLL: n     SCE: s\\nMCE y     Brier: z" - `np.around(..., 3)` and the five-space gaps included; "ACE "
    under the quantile strategy.  -> the title's two lines."""
    err = "ACE " if quantile else "ECE "
    t = report.target(target)
    ece, mce = report.ece(table, t, segment, overflow), report.mce(table, t, segment, overflow)
    if t < report.C:
        title = err + str(np.around(ece, 3)) + "\nMCE " + str(np.around(mce, 3)) + "     Brier: " + str(np.around(report.brier(table, t, segment), 3))
    else:
        title = (err + str(np.around(ece, 3)) + "     NLL: " + str(np.around(report.nll(table, segment), 3)) + "     SCE: " +
                 str(np.around(report.sce(table, segment, overflow), 3)) + "\n" + "MCE " + str(np.around(mce, 3)) + "     Brier: " +
                 str(np.around(report.brier_all(table, segment), 3)))
    return title.split("\n")


def from_filtered(filtered, models=None, split=None, edges=None, quantile=False, device=0, engine=None, overflow="raise", one_based=False):
    """The report of the matched rows `calibration.gather_detections` returns (its `gt_classes` are class - 1, the index the
    reference's ClassificationCalib takes) on the evaluation split of `_calibr_plot` (:275-322): rows `split` onwards, default
    int(0.8 * n).  models: the dict a `ClassCalibrator` takes (any of ts_all, ts_percls, iso_all, iso_percls), None: the
    uncalibrated table alone.  quantile: bin by `quantile_edges` (the reference's ACE) unless `edges` are given.  one_based: the
    rows carry the ground truth's class id, as those of `writers.validate_to_file` do: 1 is subtracted.  One segment."""
    if filtered.get("logits") is None:
        raise ValueError("class report: the matched rows carry no logits")
    logits = np.asarray(filtered["logits"])
    logits = logits.reshape(len(logits), -1)
    lab = np.asarray(filtered["gt_classes"]).reshape(-1) - (1 if one_based else 0)
    split = int(len(logits) * 0.8) if split is None else int(split)
    models = dict(models or {})
    unknown = set(models) - set(METHOD_NAMES)
    if unknown:
        raise ValueError("class report: no such calibration models: %s" % sorted(unknown))
    tables, names = tables_from_logits(logits[split:], **{k: models[k] for k in ("ts_all", "ts_percls", "iso_all", "iso_percls") if k in models})
    if edges is None and quantile:
        edges = quantile_edges(tables)
    return report(tables, lab[split:], names, None, edges, None, device, engine, overflow)
