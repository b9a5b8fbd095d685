"""Plain-numpy mirror of the contract of uda_kde_eval_np (include/uda_hip.h): the sum of Gaussian terms of every evaluation point
over a problem's whitened data rows - scipy.stats.gaussian_kde's inner loop (reference src/uncertainty_ep_vs_al.py:361-375) - with
the entry point's own arithmetic and its own order of summation.

  arg   ((p0 - d0)^2 + (p1 - d1)^2) + ... over the coordinates in ascending order, every operation rounded on its own
  term  w * exp(arg * -0.5); the multiplication is left out when there are no weights
  sum   the rows are cut into runs of RUN, aligned to the first row; a run is summed sequentially from 0.0; the run sums are
        folded as the zero-padded pairwise tree (`b = b[0::2] + b[1::2]`)

`kde_sum` is the entry point for one problem, `kde_eval_np` has the signature of `epal.kde_eval_np` and can stand in for the device
wherever that module takes `engine=`; `pdf` is the whole of gaussian_kde(dataset, bw_method, weights)(points) on the mirror.
Points go through in blocks, so nothing larger than block x n is ever held."""
import re
import os

import numpy as np

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uda_hip.h")
RUN = int(re.search(r"#define UDA_KDE_RUN (\d+)", open(_HEADER).read()).group(1))


def kde_sum(data, points, weight=None, run=RUN, block=2048):
    """data [n, D], points [m, D] float64, weight [n] or None -> sum [m]."""
    d = np.ascontiguousarray(data, np.float64).reshape(len(data), -1)
    p = np.ascontiguousarray(points, np.float64).reshape(len(points), d.shape[1])
    w = None if weight is None else np.ascontiguousarray(weight, np.float64)
    n, runs = d.shape[0], (d.shape[0] + run - 1) // run
    size = 1
    while size < runs:
        size *= 2
    out = np.empty(p.shape[0], np.float64)
    with np.errstate(under="ignore"):
        for lo in range(0, p.shape[0], block):
            rows = p[lo:lo + block]
            e = rows[:, None, 0] - d[None, :, 0]
            arg = e * e
            for k in range(1, d.shape[1]):
                e = rows[:, None, k] - d[None, :, k]
                arg = arg + e * e
            t = np.exp(arg * -0.5)
            if w is not None:
                t = w[None, :] * t
            b = np.zeros((size, rows.shape[0]), np.float64)
            for r in range(runs):
                acc = np.zeros(rows.shape[0], np.float64)
                for i in range(r * run, min(n, (r + 1) * run)):
                    acc = acc + t[:, i]
                b[r] = acc
            while len(b) > 1:
                b = b[0::2] + b[1::2]
            out[lo:lo + block] = b[0]
    return out


def kde_eval_np(D, data, d_off, weight, points, p_off, device=0):
    """The array form of the entry point: all problems of a call, one after the other."""
    out = np.empty(int(p_off[-1]), np.float64)
    for b in range(len(d_off) - 1):
        rows = slice(int(d_off[b]), int(d_off[b + 1]))
        out[int(p_off[b]):int(p_off[b + 1])] = kde_sum(np.reshape(data, (-1, D))[rows], np.reshape(points, (-1, D))[int(p_off[b]):int(p_off[b + 1])],
                                                        None if weight is None else weight[rows])
    return out


def pdf(dataset, points, weights=None, bw_method=None):
    """gaussian_kde(dataset [D, n], bw_method, weights)(points [D, m]) with scipy's own covariance, Cholesky factor, whitening and
    norm, and the mirror's sum in place of scipy's loop."""
    from scipy import linalg
    from scipy.stats import gaussian_kde
    kde = gaussian_kde(dataset, bw_method=bw_method, weights=weights)
    points = np.atleast_2d(np.asarray(points, np.float64))
    data_w = linalg.solve_triangular(kde.cho_cov, kde.dataset, lower=True).T
    points_w = linalg.solve_triangular(kde.cho_cov, points, lower=True).T
    norm = (2 * np.pi) ** (-kde.d / 2)
    for i in range(kde.d):
        norm /= kde.cho_cov[i, i]
    return kde_sum(data_w, points_w, kde.weights) * norm


GOLDEN_PARAMS = {"enable_softmax": True, "mc_boxheadrate": 0.1, "loss_attenuation": True, "calibrate_regression": True}
GOLDEN_COLUMNS = ("names", "scores", "boxes", "gt_boxes", "classes", "gt_classes", "logits", "probab", "entropy", "mcbox", "albox")


def golden_records(cols):
    """The validate_results records of one case of tests/golden/epal_golden.npz from its stored columns (a dict keyed by
    GOLDEN_COLUMNS; the iso_all
    columns are derived here), through `writers.validate_records` - the records make_epal_golden.py wrote for the reference to read."""
    from uda_amd import writers
    n = len(cols["boxes"])
    filtered = {k: cols[k] for k in ("scores", "boxes", "gt_boxes", "logits", "probab", "entropy", "mcbox", "albox")}
    filtered.update(names=[str(v) for v in cols["names"]], occlusions=[0] * n, truncations=[0.0] * n,
                    classes=[int(v) for v in cols["classes"]], gt_classes=[int(v) for v in cols["gt_classes"]])
    def grid(a):                                               # the "calibrated" sigmas: an affine map, back onto the 1/1024 grid
        return (np.round(a * 1024.0) / 1024.0).astype(np.float32)

    calibrated = {"iso_all_mcbox": grid(np.asarray(cols["mcbox"], np.float64) * 1.75 + 0.25),
                  "iso_all_albox": grid(np.asarray(cols["albox"], np.float64) * 0.625 + 0.125)}
    return writers.validate_records(filtered, GOLDEN_PARAMS, calibrated)


def golden_case(gold, case):
    return golden_records({k: gold["%s_%s" % (case, k)] for k in GOLDEN_COLUMNS})
