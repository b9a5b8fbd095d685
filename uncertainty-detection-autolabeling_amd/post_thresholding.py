"""Post-thresholding analysis: where in the image and on which images the failure-recognition threshold acts - the three steps that
close `MainUncertViz.__init__` (reference uncertainty_analysis.py:502-508, defined at :838-880 and :920-1068), as arrays and numbers;
nothing is drawn.

  box_slices        (y1, x1, y2, x2) float64 boxes -> the half-open (r0, r1, c0, c1) ranges `mask[int(y1):int(y2), int(x1):int(x2)]`
                    resolves to on a map of H x W
  heat_np           the raw device call (`uda_heat_maps_np`): M maps from rectangle sets, value columns and row selectors
  heat_maps         `_plot_validheat` (:920-1019): the ten maps the reference hands to imshow, keyed by its file stems, from ONE call
  post_np           the raw tally call (`uda_thr_post_np`)
  spider_metrics    `_plot_metricsspider` (:1024-1068): `collected_data` [3, 5] - all / removed / remaining x mIoU, Acc, %Det., %CD,
                    %FD - averaged over the IoU thresholds, times 100
  rank_images       `_collect_postthresholding` (:838-880): the images with the most correctly removed, falsely removed and falsely
                    remaining rows, and random images on which nothing is removed
  post_threshold_analysis   the three steps after `thresholding.collect_thresh_results`, in one call

Not built: the drawing itself (imshow, the polar plot, `_draw_postthresholding`) and the per-class heat maps the reference has
commented out (:1021-1022).
"""
import random as _random

import numpy as np

from . import capi
from . import thresholding as TH

TILE_H, TILE_W, CHUNK = capi.HEAT_TILE_H, capi.HEAT_TILE_W, capi.HEAT_CHUNK
MAX_MAPS, MAX_RECTS, MAX_VALUES, MAX_SELS, MAX_PIXELS = (capi.HEAT_MAX_MAPS, capi.HEAT_MAX_RECTS, capi.HEAT_MAX_VALUES,
                                                         capi.HEAT_MAX_SELS, capi.HEAT_MAX_PIXELS)
MAX_N, MAX_K = capi.THR_MAX_N, capi.THR_MAX_THRS
HEAT_KEYS = ("gt_loc", "uncert_albox", "rmse_albox", "uncert_calib_albox", "rmse_calib_albox", "entropy", "calib_entropy",
             "opt_uncert_cr", "opt_uncert_fr", "opt_uncert_fk")
LIST_KEYS = ("top_correctremove", "top_falserremove", "top_falseremain", "random_noremoval")

_ptr = TH._ptr


def _resolve(v, size):
    """A slice bound int(v) on an axis of `size`: truncation toward zero, a negative index counts from the end and clamps at 0,
    a positive one clamps at the size."""
    t = np.trunc(v)
    return np.where(t < 0, np.maximum(t + size, 0.0), np.minimum(t, float(size))).astype(np.int32)


def box_slices(boxes, H, W):
    """[N, 4] (y1, x1, y2, x2) -> int32 [N, 4] (r0, r1, c0, c1), exactly the ranges `mask[int(y1):int(y2), int(x1):int(x2)]`
    covers on an H x W mask (`slice(int(a), int(b)).indices(size)`); r1 <= r0 or c1 <= c0 covers nothing.  A non-finite
    coordinate raises ValueError (the reference's int() raises too)."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    if not np.isfinite(b).all():
        raise ValueError("a box coordinate is NaN or inf")
    H, W = int(H), int(W)
    return np.ascontiguousarray(np.stack([_resolve(b[:, 0], H), _resolve(b[:, 2], H), _resolve(b[:, 1], W), _resolve(b[:, 3], W)],
                                         axis=1))


def check_heat_problem(rects, values, sel, map_rect, map_value, map_sel, map_mean, H, W):
    """Contiguous arrays of the types `uda_heat_maps_np` takes; ValueError for a shape, a non-finite value, an index outside its
    table, a rectangle outside the map or a limit."""
    rects = np.asarray(rects)
    if rects.ndim == 2:
        rects = rects[None]
    if rects.ndim != 3 or rects.shape[2] != 4:
        raise ValueError("rects must be [R, N, 4], got shape %s" % (rects.shape,))
    if not np.array_equal(rects, np.round(rects)):
        raise ValueError("rects must hold whole numbers")
    R, N = rects.shape[:2]
    if not 1 <= R <= MAX_RECTS:
        raise ValueError("%d rectangle sets: 1..%d are taken" % (R, MAX_RECTS))
    if not 1 <= N <= MAX_N:
        raise ValueError("%d rows: 1..%d are taken" % (N, MAX_N))
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W > MAX_PIXELS:
        raise ValueError("a map of %d x %d: at least 1 x 1 and at most %d pixels are taken" % (H, W, MAX_PIXELS))
    if (rects < 0).any() or (rects[..., :2] > H).any() or (rects[..., 2:] > W).any():
        raise ValueError("a rectangle lies outside the %d x %d map" % (H, W))
    rects = np.ascontiguousarray(rects.astype(np.int32))
    values = np.zeros((0, N), np.float64) if values is None else np.ascontiguousarray(np.asarray(values, np.float64))
    if values.ndim == 1:
        values = values[None] if values.size else values.reshape(0, N)
    sel = np.zeros((0, N), np.uint8) if sel is None else np.asarray(sel)
    if sel.ndim == 1:
        sel = sel[None] if sel.size else sel.reshape(0, N)
    if values.ndim != 2 or values.shape[1] != N or sel.ndim != 2 or sel.shape[1] != N:
        raise ValueError("values %s and sel %s must be [V, %d] and [Q, %d]" % (values.shape, sel.shape, N, N))
    sel = np.ascontiguousarray(sel.astype(bool).astype(np.uint8))
    V, Q = values.shape[0], sel.shape[0]
    if V > MAX_VALUES or Q > MAX_SELS:
        raise ValueError("%d value columns and %d selectors: at most %d and %d are taken" % (V, Q, MAX_VALUES, MAX_SELS))
    TH._finite(values, "values")
    tabs = [np.asarray(t).reshape(-1) for t in (map_rect, map_value, map_sel, map_mean)]
    M = tabs[0].size
    if not 1 <= M <= MAX_MAPS or any(t.size != M for t in tabs):
        raise ValueError("the four map tables hold %s entries: 1..%d each, all alike, are taken" % ([t.size for t in tabs], MAX_MAPS))
    if any(not np.array_equal(t, np.round(t)) for t in tabs):
        raise ValueError("the map tables must hold whole numbers")
    tabs = [np.ascontiguousarray(t.astype(np.int32)) for t in tabs]
    for t, lo, hi, what in ((tabs[0], 0, R, "rectangle set"), (tabs[1], -1, V, "value column"), (tabs[2], -1, Q, "selector")):
        if (t < lo).any() or (t >= hi).any():
            raise ValueError("a map reads a %s outside %d..%d" % (what, lo, hi - 1))
    return (rects, values, sel) + tuple(tabs) + (H, W)


def heat_np(rects, values, sel, map_rect, map_value, map_sel, map_mean, H, W, device=0, count=True):
    """The raw device call: (heat [M, H, W] float64, count [M, H, W] int32 or None) of `uda_heat_maps_np`.  rects [R, N, 4] int32
    (r0, r1, c0, c1); values [V, N] or None; sel [Q, N] or None; map m reads rectangle set map_rect[m], value column map_value[m]
    (-1: 1.0) and selector map_sel[m] (-1: every row), and with map_mean[m] holds sum / count (+0.0 where nothing covers)."""
    rects, values, sel, m_rect, m_value, m_sel, m_mean, H, W = check_heat_problem(rects, values, sel, map_rect, map_value, map_sel,
                                                                                   map_mean, H, W)
    (R, N), V, Q, M = rects.shape[:2], values.shape[0], sel.shape[0], m_rect.size
    heat = np.zeros((M, H, W), np.float64)
    cnt = np.zeros((M, H, W), np.int32) if count else None
    lib = capi.load()
    rc = lib.uda_heat_maps_np(int(device), _ptr(rects), R, _ptr(values) if V else None, V, _ptr(sel) if Q else None, Q, N,
                              _ptr(m_rect), _ptr(m_value), _ptr(m_sel), _ptr(m_mean), M, H, W, _ptr(heat),
                              _ptr(cnt) if count else None)
    capi.check(lib, None, rc, "uda_heat_maps_np")
    return heat, cnt


def heat_maps(gt_boxes, pred_boxes, mask_size, albox=None, calib_albox=None, entropy=None, calib_entropy=None, opt_uncert=None,
              pred_filters=None, device=0, heat=None):
    """`_plot_validheat` (:920-1019) without the drawing: a dict of [H, W] float64 maps keyed by the reference's file stems
    (HEAT_KEYS) - the arrays it hands to imshow.  gt_boxes / pred_boxes [N, 4] (y1, x1, y2, x2); mask_size (H, W); albox /
    calib_albox [N, 4] relative sigma; entropy / calib_entropy [N]; opt_uncert [N] with pred_filters, the three masks
    `thresholding.collect_thresh_results` returns (a fourth entry, the threshold, is ignored).  Only the maps whose inputs are given
    are returned, and all of them come from one device call: the value columns are the reference's own numpy expressions, the three
    filter maps select rows instead of copying boxes.  heat: a stand-in for `heat_np` with its signature (tests inject the mirror)."""
    H, W = int(mask_size[0]), int(mask_size[1])
    gt, pred = np.asarray(gt_boxes, np.float64).reshape(-1, 4), np.asarray(pred_boxes, np.float64).reshape(-1, 4)
    if gt.shape != pred.shape:
        raise ValueError("gt_boxes of %d rows and pred_boxes of %d" % (len(gt), len(pred)))
    N = len(gt)
    rects = np.stack([box_slices(gt, H, W), box_slices(pred, H, W)])
    GT, PRED = 0, 1
    values, sels, maps = [], [], []          # maps: (key, rectangle set, value column, selector, mean)

    def column(v):
        v = np.asarray(v, np.float64).reshape(-1)
        if v.size != N:
            raise ValueError("a column of %d rows for boxes of %d" % (v.size, N))
        values.append(v)
        return len(values) - 1

    maps.append(("gt_loc", GT, -1, -1, 0))
    for al, stem in ((albox, "albox"), (calib_albox, "calib_albox")):
        if al is not None:
            al = np.asarray(al, np.float64).reshape(N, 4)
            maps.append(("uncert_" + stem, PRED, column(np.mean(al, axis=1)), -1, 1))
            maps.append(("rmse_" + stem, GT, column(np.sqrt(np.mean((np.abs(gt - pred) - al) ** 2, axis=-1))), -1, 1))
    for ent, key in ((entropy, "entropy"), (calib_entropy, "calib_entropy")):
        if ent is not None:
            maps.append((key, PRED, column(ent), -1, 1))
    if opt_uncert is not None and pred_filters is not None:
        col = column(opt_uncert)
        for f, key in zip(pred_filters[:3], ("opt_uncert_cr", "opt_uncert_fr", "opt_uncert_fk")):
            f = np.asarray(f).reshape(-1)
            if f.size != N:
                raise ValueError("a filter of %d rows for boxes of %d" % (f.size, N))
            sels.append(f.astype(bool))
            maps.append((key, PRED, col, len(sels) - 1, 1))
    out, _ = (heat or heat_np)(rects, np.stack(values) if values else None, np.stack(sels) if sels else None,
                               [m[1] for m in maps], [m[2] for m in maps], [m[3] for m in maps], [m[4] for m in maps], H, W,
                               device=device, count=False)
    return {m[0]: (np.nan_to_num(out[j], copy=False) if m[4] else out[j]) for j, m in enumerate(maps)}


def check_post_problem(u, ious, tp_class, iou_thrs, thrs, image=None, k_img=-1):
    """Contiguous arrays of the types `uda_thr_post_np` takes; ValueError for a shape, a NaN or a limit.  Returns (u, ious, tp,
    iou_thrs, thrs, image or None, I, k_img)."""
    u = np.ascontiguousarray(np.asarray(u, np.float64).reshape(-1))
    N = u.size
    if not 2 <= N <= MAX_N:
        raise ValueError("%d rows: 2..%d are taken" % (N, MAX_N))
    ious = np.ascontiguousarray(np.asarray(ious, np.float64).reshape(-1))
    tp = np.ascontiguousarray(np.asarray(tp_class).reshape(-1).astype(bool).astype(np.uint8))
    if ious.size != N or tp.size != N:
        raise ValueError("ious of %d rows and tp_class of %d for scores of %d" % (ious.size, tp.size, N))
    iou_thrs = np.ascontiguousarray(np.asarray(iou_thrs, np.float64).reshape(-1))
    thrs = np.ascontiguousarray(np.asarray(thrs, np.float64).reshape(-1))
    K = iou_thrs.size
    if not 1 <= K <= MAX_K or thrs.size != K:
        raise ValueError("%d IoU thresholds and %d thresholds: 1..%d of each, as many of one as of the other, are taken"
                         % (K, thrs.size, MAX_K))
    for a, what in ((u, "the scores"), (ious, "ious"), (iou_thrs, "iou_thrs"), (thrs, "thrs")):
        if np.isnan(a).any():
            raise ValueError("%s hold NaN" % what)
    k_img, I = int(k_img), 0
    if not -1 <= k_img < K:
        raise ValueError("k_img %d: -1..%d are taken" % (k_img, K - 1))
    if k_img >= 0:
        if image is None:
            raise ValueError("k_img %d without image ids" % k_img)
        ids = np.asarray(image).reshape(-1)
        if ids.size != N:
            raise ValueError("image ids of %d rows for scores of %d" % (ids.size, N))
        if not np.array_equal(ids, np.round(ids)) or ids.min() < 0 or ids.max() >= N:
            raise ValueError("image ids must be whole numbers in 0..%d" % (N - 1))
        image = np.ascontiguousarray(ids.astype(np.int32))
        I = int(image.max()) + 1
    else:
        image = None
    return u, ious, tp, iou_thrs, thrs, image, I, k_img


def post_np(u, ious, tp_class, iou_thrs, thrs, image=None, k_img=-1, device=0):
    """The raw tally call: (counts [K, 2, 4] int64, iou_sum [K, 2], img_count [I, 4] int32, img_first [I, 3] int32) of
    `uda_thr_post_np`; side 0 is u >= thrs[k] (removed), side 1 u < thrs[k] (remaining); counts: rows, tp_class rows, correct
    rows, wrong rows.  With k_img >= 0 and image [N] (ids 0..I-1, I = the largest id + 1) the per-image outputs are taken at
    threshold k_img: correctly removed, falsely removed, falsely remaining rows and rows with u >= thr, and the first row of each
    of the three kinds (N: none); else both are None."""
    u, ious, tp, iou_thrs, thrs, image, I, k_img = check_post_problem(u, ious, tp_class, iou_thrs, thrs, image, k_img)
    N, K = u.size, thrs.size
    counts, iou_sum = np.zeros((K, 2, 4), np.int64), np.zeros((K, 2), np.float64)
    img_count = np.zeros((I, 4), np.int32) if k_img >= 0 else None
    img_first = np.zeros((I, 3), np.int32) if k_img >= 0 else None
    lib = capi.load()
    rc = lib.uda_thr_post_np(int(device), _ptr(u), _ptr(ious), _ptr(tp), _ptr(image) if image is not None else None, N, I,
                             _ptr(iou_thrs), _ptr(thrs), K, k_img, _ptr(counts), _ptr(iou_sum),
                             _ptr(img_count) if img_count is not None else None, _ptr(img_first) if img_first is not None else None)
    capi.check(lib, None, rc, "uda_thr_post_np")
    return counts, iou_sum, img_count, img_first


def _threshold(u, ious, tp, iou_thrs, s, device, report):
    """The thresholds roc_metrics gives opt_uncert at every IoU threshold: `thr_report` with one score column."""
    rep = TH.thr_report(u[None], ious, tp, iou_thrs, s["thr_cd"], s["thr_fpr_tpr"], device=device, report=report)
    return np.ascontiguousarray(rep.thr[0, 0])


def spider_metrics(opt_uncert, ious, tps_class, params=None, device=0, report=None, post=None):
    """`_plot_metricsspider` (:1024-1068) without the plot: `collected_data` as a [3, 5] array - rows all / removed / remaining
    detections, columns mIoU, Acc, %Det., %CD, %FD -, the mean over the IoU thresholds `thr_iou_thrs` times 100.  The threshold of
    every IoU threshold comes from `thr_report`, the tallies from one `post_np` call; the ratios are the reference's own float64
    divisions, so an empty side or a zero denominator gives what numpy gives (NaN / inf), warnings silenced.  Only the two sums of
    IoU are ordered differently from numpy's.  report / post: stand-ins for `thresholding.report_np` / `post_np`."""
    s = TH._settings(params)
    u = np.asarray(opt_uncert, np.float64).reshape(-1)
    ious, tp = np.asarray(ious, np.float64).reshape(-1), np.asarray(tps_class).reshape(-1).astype(bool)
    iou_thrs = [float(t) for t in s["thr_iou_thrs"]]
    thrs = _threshold(u, ious, tp, iou_thrs, s, device, report)
    counts, iou_sum, _, _ = (post or post_np)(u, ious, tp, iou_thrs, thrs, device=device)
    n = counts.astype(np.float64)
    all_rows = np.array([np.mean(ious), np.mean(tp), 1, 1, 1], np.float64)
    with np.errstate(all="ignore"):
        correct, wrong = n[:, 0, 2] + n[:, 1, 2], n[:, 0, 3] + n[:, 1, 3]
        sides = [np.stack([iou_sum[:, j] / n[:, j, 0], n[:, j, 1] / n[:, j, 0], n[:, j, 0] / np.float64(u.size), n[:, j, 2] / correct,
                           n[:, j, 3] / wrong], axis=1) for j in (0, 1)]
        return np.stack([np.mean(np.tile(all_rows, (len(iou_thrs), 1)), axis=0) * 100, np.mean(sides[0], axis=0) * 100,
                         np.mean(sides[1], axis=0) * 100])


def rank_images(image_names, opt_uncert, ious, tps_class, eval_iou_thr, params=None, top=10, rng=None, device=0, report=None,
                post=None):
    """`_collect_postthresholding` (:838-880) without the drawing: a dict of four lists of image names (LIST_KEYS) - the `top`
    images with the most correctly removed, falsely removed and falsely remaining rows at the IoU threshold eval_iou_thr, in
    `Counter.most_common(top)` order (count descending, ties to the image whose first such row comes first), and `top` images on
    which no row is removed, drawn with `rng.sample(range(n), top)` from those images in `np.unique` order.  rng: a
    `random.Random`; the default is the `random` module, as in the reference.  With fewer than `top` such images the reference
    raises ValueError (random.sample of a larger sample than population); this function takes min(top, n) of them instead."""
    s = TH._settings(params)
    u = np.asarray(opt_uncert, np.float64).reshape(-1)
    ious, tp = np.asarray(ious, np.float64).reshape(-1), np.asarray(tps_class).reshape(-1).astype(bool)
    names, ids = np.unique(np.asarray(image_names), return_inverse=True)
    ids = ids.reshape(-1)
    if ids.size != u.size:
        raise ValueError("%d image names for scores of %d" % (ids.size, u.size))
    thr = _threshold(u, ious, tp, [float(eval_iou_thr)], s, device, report)
    _, _, img_count, img_first = (post or post_np)(u, ious, tp, [float(eval_iou_thr)], thr, image=ids, k_img=0, device=device)
    out = {}
    for j, key in enumerate(LIST_KEYS[:3]):
        has = np.flatnonzero(img_count[:, j] > 0)
        order = has[np.lexsort((img_first[has, j], -img_count[has, j].astype(np.int64)))]
        out[key] = [str(v) for v in names[order[:top]]]
    kept = names[img_count[:, 3] == 0]
    picks = (rng or _random).sample(range(len(kept)), min(int(top), len(kept)))
    out[LIST_KEYS[3]] = [str(v) for v in kept[picks]]
    return out


def post_threshold_analysis(gt_boxes, pred_boxes, mask_size, image_names, opt_uncert, ious, tps_class, params=None, albox=None,
                            calib_albox=None, entropy=None, calib_entropy=None, top=10, rng=None, device=0, heat=None, report=None,
                            post=None):
    """The three steps the reference lists after the search (:502-508) for a caller who holds the arrays of
    `thresholding.from_validate_records` and the boxes: `collect_thresh_results` at the largest IoU threshold, then
    `spider_metrics`, `rank_images` and `heat_maps`.  Returns {"heat": ..., "spider": ..., "images": ...}."""
    s = TH._settings(params)
    eval_iou_thr = float(np.max(s["thr_iou_thrs"]))
    filters = TH.collect_thresh_results(opt_uncert, ious, tps_class, eval_iou_thr, params=params, device=device, report=report)
    spider = spider_metrics(opt_uncert, ious, tps_class, params=params, device=device, report=report, post=post)
    images = rank_images(image_names, opt_uncert, ious, tps_class, eval_iou_thr, params=params, top=top, rng=rng, device=device,
                         report=report, post=post)
    maps = heat_maps(gt_boxes, pred_boxes, mask_size, albox=albox, calib_albox=calib_albox, entropy=entropy,
                     calib_entropy=calib_entropy, opt_uncert=opt_uncert, pred_filters=filters, device=device, heat=heat)
    return {"heat": maps, "spider": spider, "images": images}
