"""Numpy mirror of the contract of uda_uncert_report_np (include/uda_hip.h): the tallies behind the validation uncertainty report
for ragged segments of matched rows and K sigma columns.  Counts are taken level by level with the comparison numpy evaluates;
every float64 sum is the root of the zero-padded pairwise tree over the segment's per-row terms (`tree`), a row's term being
(t0 + t1) + (t2 + t3) of its four coordinates.  `report` has the signature and the result of `uncertainty_report.report_np`, so it
can stand in for the device wherever that module takes `engine=`."""
import numpy as np

import tree_ref

HALF_LOG_2PI = 0.9189385332046727
tree = tree_ref.tree


def levels_z(levels=100):
    from scipy import stats
    p_m = np.linspace(0, 1, int(levels))
    return p_m, stats.norm.ppf((1 - p_m) / 2)


def row_terms(t):
    """[n, 4] element terms -> [n] row terms."""
    return (t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3])


def iou(gt, pred):
    """calc_iou_np (utils_box.py:56-89) in float64, one operation at a time."""
    yA, xA = np.maximum(gt[:, 0], pred[:, 0]), np.maximum(gt[:, 1], pred[:, 1])
    yB, xB = np.minimum(gt[:, 2], pred[:, 2]), np.minimum(gt[:, 3], pred[:, 3])
    inter = np.maximum(0.0, xB - xA) * np.maximum(0.0, yB - yA)
    a = np.abs(gt[:, 3] - gt[:, 1]) * np.abs(gt[:, 2] - gt[:, 0])
    b = np.abs(pred[:, 3] - pred[:, 1]) * np.abs(pred[:, 2] - pred[:, 0])
    uni = (a + b) - inter
    return np.divide(inter, uni, out=np.zeros_like(inter), where=uni != 0)


def nll_terms(res, s):
    """The element terms of S_nll and the degenerate mask; a degenerate element's term is 0."""
    bad = (s == 0) | ~np.isfinite(s)
    safe = np.where(bad, 1.0, s)
    y = res / safe
    return np.where(bad, 0.0, (y * y / 2.0 + np.log(safe)) + HALF_LOG_2PI), bad


def report(gt, pred, sigmas, gt_classes, classes, segments=None, levels=100, device=0, z=None):
    gt, pred = np.asarray(gt, np.float64).reshape(-1, 4), np.asarray(pred, np.float64).reshape(-1, 4)
    N = len(gt)
    sig = np.asarray(sigmas, np.float64)
    sig = sig.reshape(len(sig), N, 4)
    gc, pc = np.asarray(gt_classes, np.float64).reshape(-1), np.asarray(classes, np.float64).reshape(-1)
    off = np.asarray([0, N] if segments is None else segments, np.int64)
    if z is None:
        p_m, z = levels_z(levels)
    else:
        z, p_m = np.asarray(z, np.float64), None
    B, K, L = len(off) - 1, len(sig), len(z)
    out = dict(seg_counts=np.zeros((B, 4), np.int64), col_counts=np.zeros((B, K, 3), np.int64), ece_count=np.zeros((B, K, 4, L), np.int64),
               seg_sums=np.zeros((B, 2)), col_sums=np.zeros((B, K, 3)), off=off, p_m=p_m, z=z)
    with np.errstate(all="ignore"):
        for b in range(B):
            g, p = gt[off[b]:off[b + 1]], pred[off[b]:off[b + 1]]
            i = iou(g, p)
            d = p - g
            out["seg_counts"][b] = [len(g), np.count_nonzero(i == 0), np.count_nonzero(gc[off[b]:off[b + 1]] != pc[off[b]:off[b + 1]]),
                                    np.count_nonzero(g != 0)]
            out["seg_sums"][b] = [tree(i), tree(row_terms(np.where(g != 0, d * d, 0.0)))]
            res = np.abs(g - p)
            for k in range(K):
                s = sig[k, off[b]:off[b + 1]]
                covered = ((p - s <= g) & (g <= p + s)).all(axis=1)
                t_nll, bad = nll_terms(res, s)
                u = s - res
                out["col_counts"][b, k] = [np.count_nonzero(covered), np.count_nonzero(res != 0), np.count_nonzero(bad)]
                out["col_sums"][b, k] = [tree(row_terms(s * s)), tree(row_terms(np.where(res != 0, u * u, 0.0))), tree(row_terms(t_nll))]
                for lv in range(L):
                    out["ece_count"][b, k, :, lv] = np.count_nonzero(np.less_equal(np.abs(p - g), np.abs(s * z[lv])), axis=0)
    return out


def sum_abs_terms(gt, pred, sigma):
    """Sum of |term| of every float64 sum of one segment and column, for the summation bounds of the tests:
    -> dict S_iou, S_sqerr, S_sigma2, S_ue, S_nll, and sum |log sigma| over the elements that are not degenerate."""
    gt, pred, s = (np.asarray(a, np.float64).reshape(-1, 4) for a in (gt, pred, sigma))
    with np.errstate(all="ignore"):
        res, d = np.abs(gt - pred), pred - gt
        t_nll, bad = nll_terms(res, s)
        u = s - res
        return dict(S_iou=np.abs(iou(gt, pred)).sum(), S_sqerr=np.where(gt != 0, d * d, 0.0).sum(), S_sigma2=(s * s).sum(),
                    S_ue=np.where(res != 0, u * u, 0.0).sum(), S_nll=np.abs(t_nll).sum(),
                    log_sigma=np.abs(np.log(np.where(bad, 1.0, s))).sum())
