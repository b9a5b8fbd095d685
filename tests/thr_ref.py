"""Plain-numpy mirror of the thresholding objective (uda_thr_objective_np): the reference's `roc_metrics` on sklearn's `roc_curve`
(drop_intermediate=True, sklearn >= 1.3) and `numpy.interp`, written out step by step.  No sklearn; the trapezoid is summed
sequentially.  tests/golden/thr_golden.npz, made from the reference's own function, pins it."""
import numpy as np


def combined(uncerts, params, group=None):
    """u[i] = sum_j params[(group[i] * U +) j] * uncerts[j, i]: products rounded one by one, added left to right, zeros unsigned."""
    uncerts = np.asarray(uncerts, np.float64)
    params = np.asarray(params, np.float64)
    U = uncerts.shape[0]
    w = np.broadcast_to(params[:U, None], uncerts.shape) if group is None else params.reshape(-1, U)[np.asarray(group)].T
    u = w[0] * uncerts[0]
    for j in range(1, U):
        u = u + w[j] * uncerts[j]
    return u + 0.0


def curve(u, correct):
    """(fps, tps, thresholds) of the kept points, the point (0, 0, +inf) in front; counts are integers."""
    u = np.asarray(u, np.float64) + 0.0
    pos = np.asarray(correct).astype(bool) == 0
    order = np.argsort(-u, kind="stable")
    us, ps = u[order], pos[order]
    idx = np.flatnonzero(np.r_[us[1:] != us[:-1], True])
    tps = np.cumsum(ps.astype(np.int64))[idx]
    fps = 1 + idx - tps
    thr = us[idx]
    if len(idx) > 2:
        keep = np.r_[True, (np.diff(fps, 2) != 0) | (np.diff(tps, 2) != 0), True]
        fps, tps, thr = fps[keep], tps[keep], thr[keep]
    return np.r_[0, fps], np.r_[0, tps], np.r_[np.inf, thr]


def interp(x, xp, fp):
    j = int(np.flatnonzero(xp <= x)[-1])        # xp[0] = 0 <= x
    if j == len(xp) - 1 or xp[j] == x:
        return fp[j]
    return (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]) * (x - xp[j]) + fp[j]


def roc_metrics(u, correct, fix_cd, budget):
    """(thr, rate, auc) of one problem; (+inf, NaN, NaN) when `correct` holds one label only."""
    fps, tps, thr = curve(u, correct)
    if fps[-1] == 0 or tps[-1] == 0:
        return np.inf, np.nan, np.nan
    fpr, tpr = fps / np.float64(fps[-1]), tps / np.float64(tps[-1])
    area = np.float64(0.0)
    for j in range(1, len(fpr)):
        area = area + (fpr[j] - fpr[j - 1]) * (tpr[j] + tpr[j - 1]) / 2.0
    if fix_cd:
        rate = 1 - interp(1 - budget, fpr, tpr)
        k = int(np.argmin(np.abs(1 - tpr - rate)))
    else:
        rate = interp(budget, tpr, fpr)
        k = int(np.argmin(np.abs(fpr - rate)))
    return thr[k], rate, area


def roc_objective(uncerts, ious, tp_class, iou_thrs, params, fix_cd, budget, group=None, device=0):
    """The batched evaluator with the signature of thresholding.roc_objective: (thr, rate, auc), each [P, K]."""
    uncerts = np.asarray(uncerts, np.float64)
    ious = np.asarray(ious, np.float64)
    tp = np.asarray(tp_class).astype(bool)
    params = np.atleast_2d(np.asarray(params, np.float64))
    iou_thrs = np.asarray(iou_thrs, np.float64).reshape(-1)
    out = np.zeros((3, params.shape[0], len(iou_thrs)))
    labels = [(ious >= t) & tp for t in iou_thrs]
    for p, row in enumerate(params):
        u = combined(uncerts, row, group)
        for k, lab in enumerate(labels):
            out[:, p, k] = roc_metrics(u, lab, fix_cd, budget)
    return out[0], out[1], out[2]
