"""Generates tests/golden/gt_assign_golden.npz by running the REAL reference functions `utils_extra.gt_box_assigner`
(src/utils_extra.py:44-64) and `utils_box.calc_iou_np` (src/utils_box.py:56-89).  Their bodies are numpy only; the modules
import TensorFlow and friends at the top, which are stubbed here.  Run once in the container where /root/reference exists;
the .npz (data only) is committed and is what the tests read - /root/reference never travels to the GPU box.

    python tests/golden/make_gt_assign_golden.py

The cases are chosen so that the fixture decides the summation order of the MSE key and the tie rule and nothing else: in
every kept GT row every other key is either exactly equal to the best one (identical boxes: the padded slots, which carry
row 0's box; or an IoU of exactly 0) or further from it than rounding can move it (MSE: 64 float32 ulps of the key; IoU:
1e-9).  The generator asserts this and prints how many rows are of each kind.
"""
import os
import sys
from unittest import mock

sys.dont_write_bytecode = True          # never write into /root/reference
for name in ("tensorflow", "tensorflow_probability", "uncertainty_toolbox", "uncertainty_toolbox.viz", "absl", "absl.logging"):
    sys.modules[name] = mock.MagicMock()
sys.path.insert(0, "/root/reference/src")
import numpy as np                       # noqa: E402
import utils_box                         # noqa: E402  (the reference modules)
import utils_extra                       # noqa: E402

M = 100
METHODS = ("IoU", "MSE", "rank")
# (valid_len per image, real GT rows per image, G)
CASES = [
    ([100, 63, 1, 0], [100, 40, 12, 5], 100),
    ([37, 100, 88], [0, 7, 3], 7),
    ([12, 99], [110, 100], 130),          # G > M: the calibrate rule stops at row M, the rank branch runs past it
]


def make_dets(rng, valid_len):
    """[M, 4] float32 y1 x1 y2 x2 inside [0, 1500]; rows >= valid_len carry row 0's box (zeros when there is none)."""
    c = rng.uniform(60, 1440, (M, 2))
    hw = rng.uniform(6, 400, (M, 2))
    b = np.column_stack([c[:, 0] - hw[:, 0] / 2, c[:, 1] - hw[:, 1] / 2, c[:, 0] + hw[:, 0] / 2, c[:, 1] + hw[:, 1] / 2])
    b = np.clip(b, 0, 1500).astype(np.float32)
    if valid_len == 0:
        b[:] = 0
    else:
        b[valid_len:] = b[0]
    return b


def make_gt_row(rng, dets, valid_len, kind):
    if kind == "far" or valid_len == 0 and kind in ("copy", "jitter", "row0"):
        y, x = rng.uniform(1700, 1900, 2)
        return np.array([y, x, y + rng.uniform(5, 100), x + rng.uniform(5, 100)], np.float32)
    if kind == "degenerate":            # zero area: a line, or a point
        y, x = rng.uniform(100, 1400, 2)
        return np.array([y, x, y, x + (rng.uniform(5, 80) if rng.random() < 0.5 else 0)], np.float32)
    if kind == "row0":
        return dets[0].copy()
    k = rng.integers(0, valid_len)
    if kind == "copy":
        return dets[k].copy()
    return (dets[k] + rng.normal(0, 4, 4)).astype(np.float32)


def row_kind(keys, best, boxes, margin, zero_ties_ok):
    """'clear' | 'tie' for one key vector, or None when some key is closer to the best than `margin` without being equal."""
    other = keys != keys[best]
    if np.any(np.abs(keys[other].astype(np.float64) - np.float64(keys[best])) <= margin):
        return None
    same = np.where(~other)[0]
    for k in same:
        if not np.array_equal(boxes[k], boxes[best]) and not (zero_ties_ok and keys[best] == 0):
            return None                 # an exact tie between different boxes that is not an IoU of 0: could depend on rounding
    return "tie" if len(same) > 1 else "clear"


def judge(gt, dets):
    g = np.asarray([gt] * M)
    iou = utils_box.calc_iou_np(g, dets)
    mse = np.mean(np.square(g - dets), axis=1)
    assert iou.dtype == np.float64 and mse.dtype == np.float32
    bi, bm = int(np.argmax(iou)), int(np.argmin(mse))
    ki = row_kind(iou, bi, dets, 1e-9, True)
    km = row_kind(mse, bm, dets, 64 * float(np.spacing(mse[bm])), False)
    return ki, km


def main():
    rng = np.random.default_rng(20241016)
    out = {"n_cases": np.array([len(CASES)]), "M": np.array([M])}
    tally = {"IoU": {"clear": 0, "tie": 0}, "MSE": {"clear": 0, "tie": 0}}
    kinds = ["jitter"] * 5 + ["copy", "copy", "row0", "far", "degenerate"]
    for ci, (valid, real, G) in enumerate(CASES):
        n = len(valid)
        dets = np.stack([make_dets(rng, v) for v in valid])
        gtb = np.full((n, G, 4), -1, np.float32)
        gtc = np.full((n, G), -1, np.float32)
        for im in range(n):
            for i in range(real[im]):
                while True:
                    row = make_gt_row(rng, dets[im], valid[im], kinds[int(rng.integers(0, len(kinds)))])
                    ki, km = judge(row, dets[im])
                    if ki and km:
                        break
                gtb[im, i] = row
                gtc[im, i] = 0.0 if rng.random() < 0.1 else float(rng.integers(1, 8))    # class 0: kept by calibrate only
                tally["IoU"][ki] += 1
                tally["MSE"][km] += 1
        out["c%d_dets" % ci], out["c%d_gt_boxes" % ci], out["c%d_gt_classes" % ci] = dets, gtb, gtc
        out["c%d_valid_len" % ci] = np.asarray(valid, np.int32)
        for method in METHODS:
            for keep in ("validate", "calibrate"):
                idx = np.full((n, G), -1, np.int32)
                iou = np.zeros((n, G), np.float64)
                ok = 1
                for im in range(n):
                    rows = np.where(gtc[im] > 0)[0] if keep == "validate" else \
                        [i for i in range(min(G, M)) if gtc[im][i] >= 0]
                    for i in rows:
                        k = int(utils_extra.gt_box_assigner(method, gtb[im], dets[im], i))
                        if k >= M:              # the reference would index past the detections next (IndexError)
                            ok = 0
                            continue
                        idx[im, i] = k
                        v = utils_box.calc_iou_np([gtb[im][i]], [dets[im][k]])
                        assert v.dtype == np.float64
                        iou[im, i] = v[0]
                tag = "c%d_%s_%s" % (ci, method, keep)
                out[tag + "_idx"], out[tag + "_iou"], out[tag + "_ok"] = idx, iou, np.array([ok])
    # the padded real rows (class -1, box -1) are never kept, so they need no separation
    print("rows by kind:", tally)
    assert min(tally["IoU"]["tie"], tally["MSE"]["tie"], tally["IoU"]["clear"], tally["MSE"]["clear"]) > 20
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gt_assign_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
