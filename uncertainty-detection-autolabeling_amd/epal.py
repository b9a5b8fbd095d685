"""The epistemic-vs-aleatoric comparison of the reference (src/uncertainty_ep_vs_al.py, `EpistemicVSAleatoric`) as data, with its
Gaussian KDE on the device.

"Where do the aleatoric and the epistemic box uncertainty of a detector disagree": the matched detections of a
validate_results.txt are laid out in the plane (mean relative aleatoric sigma, mean relative MC-dropout sigma - or the
classification entropy), the plane is cut into the finest grid whose two off-diagonal corner cells still hold detections, and
the detections of the "high AL / low EP" and "low AL / high EP" corners are listed with their metrics.  The reference draws all of
it; its one expensive step is `gaussian_kde([av_al, av_mc])` on a 100 x 100 mesh (:361-375: N x 10 000 float64 Gaussian terms in
scipy's sequential loop, once per configuration).  Here that is one problem of ONE device call for all configurations (C entry
point uda_kde_eval_np: float64, a stated order of summation); everything else is O(N) and stays on the host.

  kde_eval_np     the thin array form of the entry point
  kde_eval        scipy.stats.gaussian_kde(dataset, bw_method, weights)(points) for a list of problems in one call: covariance,
                  Scott / Silverman / scalar factor, Cholesky factor, whitening and norm as scipy computes them, on the host
  cell_indices    `_get_cell_indices` (:59-74), vectorised
  find_grid       the search of `get_plot_grid` (:286-317)
  compare_epal    `compare_epal` (:456-545) -> EpalComparison
  compare_many    several (uncert, ent) configurations of one set of records, all their KDEs in one call
  writers.write_epal_highlow   the two text files of `save_highlow` (:393-449)

Not built: every drawing (`plot_unc_metrics`, the scatter, `contourf`), the crop montages of `_save_crops`, the BRISQUE column of
`get_metrics_comp` (the `brisque` package; its position in the metric lists holds None), seaborn's histogram curve of
`_plot_uncert_dist`, and `InferImages._compare_highlow_epal`, which copies files.  The switches that would select one of them
raise NotImplementedError.  scipy (linalg) is imported where it is used, as set_similarity does.
"""
import ast
import os
import warnings

import numpy as np

from . import capi
from .thresholding import calc_iou_np, relativize_uncert

MAX_D = capi.KDE_MAX_D
MAX_GRID = 64
LABELS = ("High Al-Low EP", "Low Al-High EP")                  # compare_epal:529, :541
COLORS = ("green", "red")
TREND_COLUMNS = (0, 3, 4, 5, 7, 8)                             # the columns plot_unc_metrics fits (6 is BRISQUE)


def kde_eval_np(D, data, d_off, weight, points, p_off, device=0):
    """uda_kde_eval_np on host arrays: data [d_off[-1], D] and points [p_off[-1], D] whitened float64 rows, weight [d_off[-1]] or
    None, offsets int64 ascending from 0 -> sum [p_off[-1]] float64.  Values must be finite."""
    data, points = np.ascontiguousarray(data, np.float64), np.ascontiguousarray(points, np.float64)
    d_off, p_off = np.ascontiguousarray(d_off, np.int64), np.ascontiguousarray(p_off, np.int64)
    if d_off.ndim != 1 or d_off.shape != p_off.shape or len(d_off) < 2:
        raise ValueError("d_off and p_off must be [B + 1] with B >= 1, got %s and %s" % (d_off.shape, p_off.shape))
    if data.size != int(d_off[-1]) * D or points.size != int(p_off[-1]) * D:
        raise ValueError("data and points must hold d_off[-1] x D and p_off[-1] x D values, got %d and %d for D = %d, offsets %d and %d"
                         % (data.size, points.size, D, d_off[-1], p_off[-1]))
    if weight is not None:
        weight = np.ascontiguousarray(weight, np.float64)
        if weight.shape != (int(d_off[-1]),):
            raise ValueError("weight must be [d_off[-1]] = [%d], got %s" % (d_off[-1], weight.shape))
    for a, what in ((data, "data"), (points, "points"), (weight, "weight")):
        if a is not None and not np.isfinite(a).all():
            raise ValueError("%s holds values that are not finite" % what)
    out = np.empty(int(p_off[-1]), np.float64)
    lib = capi.load()
    rc = lib.uda_kde_eval_np(int(device), int(D), len(d_off) - 1, data.ctypes.data, d_off.ctypes.data,
                             None if weight is None else weight.ctypes.data, points.ctypes.data, p_off.ctypes.data, out.ctypes.data)
    capi.check(lib, None, rc, "uda_kde_eval_np")
    return out


_SINGULAR = ("The data appears to lie in a lower-dimensional subspace of the space in which it is expressed. This has resulted in a "
             "singular data covariance matrix, which cannot be treated using the algorithms implemented in `gaussian_kde`. Consider "
             "performing principal component analysis / dimensionality reduction and using `gaussian_kde` with the transformed data.")


def _whiten(dataset, points, weights, bw_method, k):
    """One problem as gaussian_kde.__init__ / _compute_covariance / gaussian_kernel_estimate prepare it: (whitened rows [n, D],
    normalised weights or None, whitened points [m, D], the factor the sum is multiplied by)."""
    from scipy import linalg
    dataset = np.atleast_2d(np.asarray(dataset, np.float64))
    if not dataset.size > 1:
        raise ValueError("`dataset` input should have multiple elements.")
    d, n = dataset.shape
    points = np.atleast_2d(np.asarray(points, np.float64))
    if points.shape[0] != d:
        if points.shape[0] == 1 and points.shape[1] == d:      # one point passed as a row vector
            points = points.reshape(d, 1)
        else:
            raise ValueError("points have dimension %d, dataset has dimension %d" % (points.shape[0], d))
    if not np.isfinite(dataset).all() or not np.isfinite(points).all():
        raise ValueError("problem %d holds values that are not finite" % k)
    if weights is None:
        w = np.ones(n) / n                                     # scipy's own default: it reaches np.cov as aweights
    else:
        w = np.atleast_1d(weights).astype(float)
        if w.ndim != 1:
            raise ValueError("`weights` input should be one-dimensional.")
        if len(w) != n:
            raise ValueError("`weights` input should be of length n")
        if not np.isfinite(w).all():
            raise ValueError("the weights of problem %d hold values that are not finite" % k)
        w = w / np.sum(w)                                  # scipy's `sum` is numpy's
    if d > n:
        raise ValueError("Number of dimensions is greater than number of samples. This results in a singular data covariance "
                         "matrix, which cannot be treated using the algorithms implemented in `gaussian_kde`.")
    neff = 1 / np.sum(w ** 2)
    if bw_method is None or bw_method == "scott":
        factor = np.power(neff, -1. / (d + 4))
    elif bw_method == "silverman":
        factor = np.power(neff * (d + 2.0) / 4.0, -1. / (d + 4))
    elif np.isscalar(bw_method) and not isinstance(bw_method, str):
        factor = bw_method
    else:
        raise ValueError("`bw_method` should be 'scott', 'silverman' or a scalar.")
    try:
        data_cho_cov = linalg.cholesky(np.atleast_2d(np.cov(dataset, rowvar=1, bias=False, aweights=w)), lower=True)
    except linalg.LinAlgError as e:
        raise linalg.LinAlgError(_SINGULAR) from e
    cho_cov = (data_cho_cov * factor).astype(np.float64)
    data_w = linalg.solve_triangular(cho_cov, dataset, lower=True).T
    points_w = linalg.solve_triangular(cho_cov, points, lower=True).T if points.shape[1] else np.empty((0, d))
    norm = (2 * np.pi) ** (-d / 2)
    for i in range(d):                                         # scipy divides one diagonal element at a time
        norm /= cho_cov[i, i]
    if weights is None:
        return data_w, None, points_w, norm / n
    return data_w, w, points_w, norm


def kde_eval(datasets, points, weights=None, bw_method=None, device=0, engine=None):
    """[scipy.stats.gaussian_kde(datasets[k], bw_method, weights[k])(points[k]) for k] with every sum of Gaussian terms in one
    device call.  datasets[k] is [D, n_k] (or [n_k] for D = 1) and points[k] [D, m_k], as scipy takes them, one D for the call;
    weights is None or a list whose entries are None or [n_k].  A singular covariance raises scipy's LinAlgError.  The values
    differ from scipy's by the order of the sum alone.  engine: a stand-in for `kde_eval_np`."""
    datasets, points = list(datasets), list(points)
    if len(datasets) != len(points) or (weights is not None and len(weights) != len(datasets)):
        raise ValueError("datasets, points and weights must list the same problems")
    if not datasets:
        return []
    if len(datasets) > capi.KDE_MAX_B:
        raise ValueError("%d problems in one call, at most %d" % (len(datasets), capi.KDE_MAX_B))
    prep = [_whiten(datasets[k], points[k], None if weights is None else weights[k], bw_method, k) for k in range(len(datasets))]
    dims = sorted({p[0].shape[1] for p in prep})
    if len(dims) != 1:
        raise ValueError("the problems of one call share one dimension, got %s" % dims)
    if not 1 <= dims[0] <= MAX_D:
        raise ValueError("data of %d dimensions: 1..%d are taken" % (dims[0], MAX_D))
    for k, p in enumerate(prep):
        if p[0].shape[0] > capi.KDE_MAX_N:
            raise ValueError("problem %d has %d data rows, at most %d" % (k, p[0].shape[0], capi.KDE_MAX_N))
    if sum(p[0].shape[0] * p[2].shape[0] for p in prep) > capi.KDE_MAX_PAIRS:
        raise ValueError("more than %d pairs of a point and a data row in one call" % capi.KDE_MAX_PAIRS)
    d_off = np.zeros(len(prep) + 1, np.int64)
    p_off = np.zeros(len(prep) + 1, np.int64)
    d_off[1:] = np.cumsum([p[0].shape[0] for p in prep])
    p_off[1:] = np.cumsum([p[2].shape[0] for p in prep])
    weighted = any(p[1] is not None for p in prep)
    weight = np.concatenate([np.ones(p[0].shape[0]) if p[1] is None else p[1] for p in prep]) if weighted else None
    total = (engine or kde_eval_np)(dims[0], np.concatenate([p[0] for p in prep]), d_off, weight, np.concatenate([p[2] for p in prep]),
                                    p_off, device=device)
    return [total[a:b] * p[3] for a, b, p in zip(p_off[:-1], p_off[1:], prep)]


def cell_indices(grid_size, data):
    """`_get_cell_indices` (:59-74) for data [N, 2]: the cell `row * grid_size + col` of every point on a grid_size x grid_size grid
    over the data's range widened by 5 % at the upper end.  Returns the reference's tuple (cell_indices int64 [N], x_min, x_step,
    y_min, y_step).  np.floor_divide on the array is the reference's scalar `//` bit for bit.  A NaN or a zero range is refused
    (the reference dies in int(nan))."""
    data = np.asarray(data, np.float64)
    g = int(grid_size)
    if data.ndim != 2 or data.shape[1] != 2 or data.shape[0] < 1:
        raise ValueError("data must be points [N, 2] with N >= 1, got shape %s" % (data.shape,))
    if g < 1:
        raise ValueError("grid_size %d: at least 1" % g)
    if not np.isfinite(data).all():
        raise ValueError("the uncertainties hold values that are not finite")
    x_min, x_max = np.min(data[:, 0]), np.max(data[:, 0])
    y_min, y_max = np.min(data[:, 1]), np.max(data[:, 1])
    x_buffer = (x_max - x_min) * 0.05
    y_buffer = (y_max - y_min) * 0.05
    x_step = (x_max + x_buffer - x_min) / g
    y_step = (y_max + y_buffer - y_min) / g
    if not (x_step > 0 and y_step > 0):
        raise ValueError("an uncertainty has a zero range (%r..%r, %r..%r): there is no grid" % (x_min, x_max, y_min, y_max))
    row = np.minimum(np.floor_divide(data[:, 1] - y_min, y_step), g - 1).astype(np.int64)
    col = np.minimum(np.floor_divide(data[:, 0] - x_min, x_step), g - 1).astype(np.int64)
    return row * g + col, x_min, x_step, y_min, y_step


def find_grid(av_al, av_mc, min_samples=3):
    """The search of `get_plot_grid` (:286-317): start at 2 x 2; while the top-left cell (g^2 - g: low AL, high EP) or the
    bottom-right cell (g - 1: high AL, low EP) holds at least `min_samples` points, grow by one; then step back by one - a search
    that never grew stays at 2.  Returns (grid_size, the tuple of `cell_indices` at that size).  From g = 22 on the 5 % buffer
    leaves the last row and column empty, so the search ends by then; beyond MAX_GRID it raises."""
    data = np.stack([np.asarray(av_al, np.float64), np.asarray(av_mc, np.float64)], axis=-1)

    def corners_empty(g):
        cells = cell_indices(g, data)[0]
        return np.count_nonzero(cells == g * g - g) < min_samples and np.count_nonzero(cells == g - 1) < min_samples

    g = 2
    if not corners_empty(g):
        while not corners_empty(g):
            g += 1
            if g > MAX_GRID:
                raise RuntimeError("the grid search passed %d x %d with a corner cell still holding %d points" % (MAX_GRID, MAX_GRID, min_samples))
        g -= 1
    return g, cell_indices(g, data)


class EpalComparison:
    """What `EpistemicVSAleatoric.compare_epal` computes before it draws.

      uncert, ent, iou_thr, im_numbs   the configuration
      keep          bool [records]: calc_iou_np(gt_bbox, bbox) > iou_thr; everything below is over the kept rows
      records, bbox, gt_bbox           the kept records and their boxes
      raw_al, raw_mc                   mean relative aleatoric sigma | mean relative epistemic sigma, or the entropy
      grid_size, cell_indices, x_min, x_step, y_min, y_step, grid_x, grid_y   the grid and the lines drawn at x_min + i * x_step
      hal_lep_ind, lal_hep_ind         the first im_numbs rows of cell g - 1 | of cell g^2 - g
      av_al, av_mc                     raw_al, raw_mc min-max normalised
      pdf_x, pdf_y, pdf                [mesh, mesh]: np.meshgrid of the two linspaces and gaussian_kde([raw_al, raw_mc]) on it
      metrics, labels, colors          per non-empty corner the list handed to plot_unc_metrics: IoU, predicted class names,
                                       ground-truth class names, score, entropy, predicted area, None (BRISQUE), av_mc, av_al
      trends                           per corner {column: np.poly1d(np.polyfit(x, col, 3))(x)} for TREND_COLUMNS, {} for one row
    """

    @property
    def subdir(self):
        return os.path.join("compare_epal", "entropy" if self.ent else "mcdropout")

    def highlow_records(self):
        return [self.records[i] for i in self.hal_lep_ind], [self.records[i] for i in self.lal_hep_ind]


def read_records(records_or_path):
    """The records of a validate_results.txt as compare_epal reads them (:459-461), or the list itself."""
    if isinstance(records_or_path, (str, os.PathLike)):
        with open(records_or_path, "r") as f:
            return [ast.literal_eval(line.replace("inf", "2e308")) for line in f.readlines()]
    return list(records_or_path)


def _column(records, key):
    if records and key not in records[0]:
        raise ValueError("the validation records have no %r" % key)
    return [r[key] for r in records]


def _metrics(records, bbox, gt_bbox, class_names):
    """`get_metrics_comp` (:220-264) without the BRISQUE scores."""
    bbox = np.stack(bbox)
    return [calc_iou_np(gt_bbox, bbox),
            [class_names[int(r["class"] - 1)] for r in records],
            [class_names[int(r["gt_class"] - 1)] for r in records],
            [r["score"] for r in records],
            _column(records, "entropy"),
            (bbox[:, 3] - bbox[:, 1]) * (bbox[:, 2] - bbox[:, 0]),
            None]


def _trends(data):
    x = np.arange(len(data[0]))
    if len(x) <= 1:
        return {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                        # polyfit's RankWarning on fewer than four rows, as in the reference
        return {c: np.poly1d(np.polyfit(x, data[c], 3))(x) for c in TREND_COLUMNS}


def _host_part(records, class_names, im_numbs, iou_thr, uncert, ent, mesh):
    """compare_epal up to the KDE: the comparison without `pdf`, the KDE's dataset [2, N] and its positions [2, mesh * mesh]."""
    c = EpalComparison()
    c.uncert, c.ent, c.iou_thr, c.im_numbs = uncert, bool(ent), iou_thr, im_numbs
    if not records:
        raise ValueError("no validation records")
    bbox, gt_bbox = _column(records, "bbox"), _column(records, "gt_bbox")
    c.keep = calc_iou_np(gt_bbox, bbox) > iou_thr
    if not c.keep.any():
        raise ValueError("no record has an IoU above %r" % iou_thr)
    c.records = [r for r, k in zip(records, c.keep) if k]
    c.bbox, c.gt_bbox = np.asarray(bbox)[c.keep], np.asarray(gt_bbox)[c.keep]
    c.raw_al = np.mean(relativize_uncert(c.bbox, np.nan_to_num(_column(c.records, uncert + "_albox"))), axis=-1)
    if ent:
        c.raw_mc = np.asarray(_column(c.records, "entropy"))
    else:
        c.raw_mc = np.mean(relativize_uncert(c.bbox, np.nan_to_num(_column(c.records, uncert + "_mcbox"))), axis=-1)
    c.grid_size, (c.cell_indices, c.x_min, c.x_step, c.y_min, c.y_step) = find_grid(c.raw_al, c.raw_mc)
    g = c.grid_size
    c.grid_x = np.asarray([c.x_min + i * c.x_step for i in range(1, g)])
    c.grid_y = np.asarray([c.y_min + i * c.y_step for i in range(1, g)])
    c.hal_lep_ind = np.where(c.cell_indices == g - 1)[0][:im_numbs]
    c.lal_hep_ind = np.where(c.cell_indices == g ** 2 - g)[0][:im_numbs]
    c.av_al = (c.raw_al - np.min(c.raw_al)) / (np.max(c.raw_al) - np.min(c.raw_al))
    c.av_mc = (c.raw_mc - np.min(c.raw_mc)) / (np.max(c.raw_mc) - np.min(c.raw_mc))
    c.pdf_x, c.pdf_y = np.meshgrid(np.linspace(c.raw_al.min(), c.raw_al.max(), mesh), np.linspace(c.raw_mc.min(), c.raw_mc.max(), mesh))
    c.metrics, c.labels, c.colors = [], [], []
    for ind, label, color in zip((c.hal_lep_ind, c.lal_hep_ind), LABELS, COLORS):
        if len(ind) > 0:
            c.metrics.append(_metrics([c.records[i] for i in ind], c.bbox[ind], c.gt_bbox[ind], class_names) + [c.av_mc[ind], c.av_al[ind]])
            c.labels.append(label)
            c.colors.append(color)
    c.trends = [_trends(m) for m in c.metrics]
    return c, np.stack([c.raw_al, c.raw_mc]), np.vstack([c.pdf_x.ravel(), c.pdf_y.ravel()])


def compare_many(records_or_path, class_names, configs, im_numbs=10, iou_thr=0.1, mesh=100, device=0, engine=None, brisque=False,
                 draw=False, crops=False):
    """`compare_epal` for every (uncert, ent) of `configs` on one set of records: the host part of each, then all KDEs in ONE
    device call.  Returns the EpalComparisons in the order of `configs`."""
    if brisque:
        raise NotImplementedError("the BRISQUE column of get_metrics_comp is not built (the brisque package); its position holds None")
    if draw or crops:
        raise NotImplementedError("the drawings and the crop montages of EpistemicVSAleatoric are not built")
    if int(mesh) < 1:
        raise ValueError("mesh %r: at least 1" % (mesh,))
    records = read_records(records_or_path)
    parts = [_host_part(records, class_names, im_numbs, iou_thr, uncert, ent, int(mesh)) for uncert, ent in configs]
    pdfs = kde_eval([p[1] for p in parts], [p[2] for p in parts], device=device, engine=engine)
    for (c, _, _), pdf in zip(parts, pdfs):
        c.pdf = pdf.reshape(c.pdf_x.shape)
    return [p[0] for p in parts]


def compare_epal(records_or_path, class_names, im_numbs=10, iou_thr=0.1, uncert="uncalib", ent=False, mesh=100, device=0,
                 engine=None, **switches):
    """`EpistemicVSAleatoric(model, im_numbs, iou_thr, uncert, ent).compare_epal()` as data: an EpalComparison.  records_or_path:
    the records of `writers.validate_records`, or the path of a validate_results.txt."""
    return compare_many(records_or_path, class_names, [(uncert, ent)], im_numbs, iou_thr, mesh, device, engine, **switches)[0]
