"""Plain-numpy mirrors of the post-thresholding analysis (uda_heat_maps_np, uda_thr_post_np): the reference's slice `+=` loop for
the maps, the zero-padded pairwise tree of tests/thr_report_ref.py for the IoU sums, np.bincount and first occurrence for the
per-image tallies.  tests/golden/thr_post_golden.npz, made from the reference's own methods, pins them.  `heat_np` and `post_np`
have the signatures of `post_thresholding.heat_np` / `post_np`, so they can stand in for the device (`heat=`, `post=`)."""
import numpy as np

from thr_report_ref import tree_sum


def heat_np(rects, values, sel, map_rect, map_value, map_sel, map_mean, H, W, device=0, count=True):
    """`mask[r0:r1, c0:c1] += value[i]` once per selected row, in row order (uncertainty_analysis.py:931-935), per map; with
    map_mean the map is count ? mask / count : +0.0."""
    rects = np.asarray(rects)
    if rects.ndim == 2:
        rects = rects[None]
    N, M = rects.shape[1], len(map_rect)
    heat, cnt = np.zeros((M, H, W), np.float64), np.zeros((M, H, W), np.int32)
    for m in range(M):
        rc = rects[map_rect[m]]
        v = np.ones(N) if map_value[m] < 0 else np.asarray(values, np.float64).reshape(-1, N)[map_value[m]]
        on = np.ones(N, bool) if map_sel[m] < 0 else np.asarray(sel).reshape(-1, N)[map_sel[m]].astype(bool)
        for i in np.flatnonzero(on):
            r0, r1, c0, c1 = (int(x) for x in rc[i])
            heat[m, r0:r1, c0:c1] += v[i]
            cnt[m, r0:r1, c0:c1] += 1
        if map_mean[m]:
            with np.errstate(all="ignore"):
                heat[m] = np.where(cnt[m] > 0, heat[m] / cnt[m], 0.0)
    return heat, (cnt if count else None)


def fold(values):
    """s = +0.0, then s = s + v in order: what one pixel of a map holds when these rows cover it."""
    s = np.float64(0.0)
    for v in np.asarray(values, np.float64):
        s = s + v
    return s


def post_np(u, ious, tp_class, iou_thrs, thrs, image=None, k_img=-1, device=0):
    u, ious = np.asarray(u, np.float64).reshape(-1), np.asarray(ious, np.float64).reshape(-1) + 0.0      # -0.0 counts as 0.0
    tp = np.asarray(tp_class).reshape(-1).astype(bool)
    iou_thrs, thrs = np.asarray(iou_thrs, np.float64).reshape(-1), np.asarray(thrs, np.float64).reshape(-1)
    N, K = u.size, thrs.size
    counts, iou_sum = np.zeros((K, 2, 4), np.int64), np.zeros((K, 2), np.float64)
    for k in range(K):
        correct = tp & (ious >= iou_thrs[k])
        for j, side in enumerate((u >= thrs[k], u < thrs[k])):
            counts[k, j] = side.sum(), (side & tp).sum(), (side & correct).sum(), (side & ~correct).sum()
            iou_sum[k, j] = tree_sum(np.where(side, ious, 0.0))
    if k_img < 0:
        return counts, iou_sum, None, None
    ids = np.asarray(image).reshape(-1).astype(np.int64)
    I = int(ids.max()) + 1
    correct, removed = tp & (ious >= iou_thrs[k_img]), u >= thrs[k_img]
    kinds = (removed & ~correct, removed & correct, (u < thrs[k_img]) & ~correct)
    img_count, img_first = np.zeros((I, 4), np.int32), np.full((I, 3), N, np.int32)
    for j, kind in enumerate(kinds):
        img_count[:, j] = np.bincount(ids[kind], minlength=I)
        rows = np.flatnonzero(kind)
        np.minimum.at(img_first[:, j], ids[rows], rows.astype(np.int32))
    img_count[:, 3] = np.bincount(ids[removed], minlength=I)
    return counts, iou_sum, img_count, img_first
