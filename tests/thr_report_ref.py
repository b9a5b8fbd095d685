"""Plain-numpy mirror of the thresholding report (uda_thr_report_np): per (segment of rows, score column, IoU threshold) the curve
of tests/thr_ref.py on the segment's rows, the label counts, the moments behind calc_jsd as the stated zero-padded pairwise tree,
and the removal counts against the threshold the curve gave.  No sklearn, no scipy.  tests/golden/thr_report_golden.npz, made from
the reference's own functions, pins it.  `report_np` has the signature of `thresholding.report_np`, so it can stand in for the
device (`report=`)."""
import numpy as np

import thr_ref
import tree_ref

tree_sum = tree_ref.tree


def roc_metrics(u, correct, fix_cd, budget):
    """thr_ref.roc_metrics with the trapezoid summed by numpy (pairwise) instead of term by term: the same thr and rate, auc
    within the bound of any order of summation, and quick at 262144 rows.  Fewer than two rows: (+inf, NaN, NaN)."""
    if len(u) < 2:
        return np.inf, np.nan, np.nan
    fps, tps, thr = thr_ref.curve(u, correct)
    if fps[-1] == 0 or tps[-1] == 0:
        return np.inf, np.nan, np.nan
    fpr, tpr = fps / np.float64(fps[-1]), tps / np.float64(tps[-1])
    area = np.sum((fpr[1:] - fpr[:-1]) * (tpr[1:] + tpr[:-1]) / 2.0)
    if fix_cd:
        rate = 1 - thr_ref.interp(1 - budget, fpr, tpr)
        k = int(np.argmin(np.abs(1 - tpr - rate)))
    else:
        rate = thr_ref.interp(budget, tpr, fpr)
        k = int(np.argmin(np.abs(fpr - rate)))
    return thr[k], rate, area


def moments(u, subset):
    """(sum, m2) of the rows of `subset` within the segment u: rows outside contribute +0.0; mean = sum / n, one division; the
    difference and the square each rounded.  An empty subset gives 0, 0."""
    n = int(np.count_nonzero(subset))
    if n == 0:
        return 0.0, 0.0
    total = tree_sum(np.where(subset, u, 0.0))
    mean = total / np.float64(n)
    d = u - mean
    return total, tree_sum(np.where(subset, d * d, 0.0))


def report_np(scores, ious, tp_class, iou_thrs, fix_cd, budget, seg_lo, seg_hi, device=0):
    scores = np.asarray(scores, np.float64) + 0.0             # -0.0 counts as 0.0
    if scores.ndim == 1:
        scores = scores[None]
    ious, tp = np.asarray(ious, np.float64).reshape(-1), np.asarray(tp_class).reshape(-1).astype(bool)
    thrs = np.asarray(iou_thrs, np.float64).reshape(-1)
    lo, hi = np.asarray(seg_lo).reshape(-1), np.asarray(seg_hi).reshape(-1)
    B, S, K = lo.size, scores.shape[0], thrs.size
    roc, n_label = np.zeros((B, S, K, 3)), np.zeros((B, K, 2), np.int64)
    mom, removed = np.zeros((B, S, K, 2, 2)), np.zeros((B, S, K, 3), np.int64)
    labels = [(ious >= t) & tp for t in thrs]
    for b in range(B):
        for k in range(K):
            correct = labels[k][lo[b]:hi[b]]
            n_label[b, k] = np.count_nonzero(correct), np.count_nonzero(~correct)
            for s in range(S):
                u = scores[s, lo[b]:hi[b]]
                roc[b, s, k] = roc_metrics(u, correct, fix_cd, budget)
                mom[b, s, k, 0], mom[b, s, k, 1] = moments(u, correct), moments(u, ~correct)
                t = roc[b, s, k, 0]
                removed[b, s, k] = (np.count_nonzero(~correct & (u >= t)), np.count_nonzero(correct & (u >= t)),
                                    np.count_nonzero(~correct & (u < t)))
    return roc, n_label, mom, removed


def mean_std(mom, n_label):
    """mean and std [B, S, K, 2] from the moments, as thresholding.ThrReport forms them; NaN for an empty subset."""
    n = n_label[:, None, :, :].astype(np.float64)
    with np.errstate(all="ignore"):
        return mom[..., 0] / n, np.sqrt(mom[..., 1] / n)


def metrics_text(jsd, auc100, fdcd, metric):
    """The text of thr_metrics_*.txt (uncertainty_analysis.py:719-730) from [U + 1, K] arrays: the U uncertainties, then the
    optimal combination."""
    lines = ["JSD, AUC, " + metric + " of Each Uncertainty:\n"]
    for idx in range(len(jsd) - 1):
        lines.append("Uncertainty %d: JSD = %.3f, AUC = %.3f, %s = %.3f\n" % (idx + 1, np.mean(jsd[idx]), np.mean(auc100[idx]), metric,
                                                                            np.mean(fdcd[idx])))
    lines.append("\nJSD, AUC, " + metric + " of Optimal Uncertainty:\n")
    lines.append("JSD = %.3f, AUC = %.3f, %s = %.3f\n" % (np.mean(jsd[-1]), np.mean(auc100[-1]), metric, np.mean(fdcd[-1])))
    return "".join(lines)
