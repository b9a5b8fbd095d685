"""The thresholding report on the device (`thresholding.report_np` -> `uda_thr_report_np`; reference
uncertainty_analysis.py:517-749, utils_extra.py:25-36) against the numpy mirror (tests/thr_report_ref.py): every integer equal,
thr / rate / sum / m2 bit for bit, auc within N * 2^-52 - at the wave, block and tile boundaries, on ragged,
nested, overlapping, repeated and degenerate segments, across a chunk of columns, at the row limit - and every case of
tests/golden/thr_report_golden.npz (what the reference's own functions returned) through the device."""
import os

import numpy as np
import pytest

import test_thr_report_host as H
import thr_ref
import thr_report_ref as RR
from uda_amd import capi
from uda_amd import thresholding as TH

pytestmark = pytest.mark.gpu

DEFAULT6 = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75]


def problem(N, S, seed=0, decimals=2):
    rng = np.random.default_rng(seed)
    tp = rng.random(N) < 0.85
    ious = np.round(rng.uniform(0.05, 0.999, N), 3)
    wrong = ~(tp & (ious >= 0.5))
    scores = np.stack([np.round(rng.uniform(0, 1.2, N) * np.where(wrong, 1.0, 0.6), decimals)] +
                      [np.round(rng.gamma(2.0, 0.05 * (s + 1), N) * np.where(wrong, 1.5, 1.0), decimals + 1) for s in range(S - 1)])
    return scores, ious, tp


def compare(got, want, n_rows):
    roc, n_label, mom, removed = got
    w_roc, w_label, w_mom, w_removed = want
    assert np.array_equal(n_label, w_label) and np.array_equal(removed, w_removed)
    for j, name in ((0, "thr"), (1, "rate")):
        a, b = roc[..., j], w_roc[..., j]
        print(name, "differing entries:", int(np.sum(~((a == b) | (np.isnan(a) & np.isnan(b))))))
        assert np.array_equal(a, b, equal_nan=True), name
    for j, name in ((0, "sum"), (1, "m2")):
        a, b = mom[..., j], w_mom[..., j]
        print(name, "differing entries:", int(np.sum(a != b)), "largest relative difference",
              float(np.max(np.abs(a - b) / np.abs(b).clip(1e-300))))
        assert np.array_equal(a, b), name
    auc, ref = roc[..., 2], w_roc[..., 2]
    assert np.array_equal(np.isnan(auc), np.isnan(ref))
    ok = ~np.isnan(ref)
    err = np.abs(auc[ok] - ref[ok]).max() if ok.any() else 0.0
    print("auc error %.3g of the bound %.3g" % (err, n_rows * 2.0 ** -52))
    assert err <= n_rows * 2.0 ** -52


def both(scores, ious, tp, thrs, fix_cd, budget, lo, hi):
    args = (scores, ious, tp, thrs, fix_cd, budget, lo, hi)
    got, want = TH.report_np(*args), RR.report_np(*args)
    compare(got, want, scores.shape[-1])
    return got


def ragged_segments(N):
    segs = [(0, N), (0, 0), (N, N), (0, 1), (N - 1, N), (0, N - 1), (1, N), (0, N)]                  # whole (twice), empty, one row
    segs += [(lo, N) for lo in (63, 2047, 2049) if lo < N] + [(lo, min(lo + 300, N)) for lo in (63, 2047, 2049) if lo < N]
    segs += [(N // 4, N // 2), (N // 3, 2 * N // 3), (N // 4 + 1, N // 2 - 1 if N >= 8 else N // 2)]   # nested, overlapping
    if N >= 6:
        segs.append((N - 4, N - 2))                                                                 # two equal rows
    return np.array(segs, np.int32)


@pytest.mark.parametrize("N", [2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097])
def test_row_counts_at_the_boundaries(N):
    scores, ious, tp = problem(N, 2, seed=N)
    if N >= 6:
        scores[:, N - 3] = scores[:, N - 4]
        tp[N - 4], ious[N - 4], tp[N - 3] = True, 0.99, False
    scores[0, 0] = -0.0
    segs = ragged_segments(N)
    roc, n_label, mom, removed = both(scores, ious, tp, [0.5, 0.75], N % 2 == 0, 0.95 if N % 3 else 0.8, segs[:, 0], segs[:, 1])
    assert np.array_equal(n_label.sum(-1), np.repeat((segs[:, 1] - segs[:, 0])[:, None], 2, 1))
    short = segs[:, 1] - segs[:, 0] < 2
    assert np.isposinf(roc[short, ..., 0]).all() and np.isnan(roc[short, ..., 1:]).all()
    assert (removed[short, ..., :2] == 0).all() and (mom[segs[:, 1] == segs[:, 0]] == 0).all()
    # the two whole-table segments carry the same bits
    for a in (roc, n_label, mom, removed):
        assert a[0].tobytes() == a[7].tobytes()


@pytest.mark.parametrize("S, K", [(1, 1), (8, 32), (1, 32), (8, 1)])
def test_column_and_threshold_counts(S, K):
    N = 300
    scores, ious, tp = problem(N, S, seed=S * 100 + K)
    thrs = [0.5] if K == 1 else np.linspace(0.05, 0.95, K)
    both(scores, ious, tp, thrs, K == 1, 0.9, [0, 10, 150], [N, 140, 299])


def test_row_limit():
    N = capi.THR_MAX_N
    scores, ious, tp = problem(N, 1, seed=7, decimals=4)
    both(scores, ious, tp, [0.5], True, 0.95, [0, 2049], [N, N - 1])


def test_a_chunk_of_columns_is_crossed():
    """8 columns of 32768 rows and 32 thresholds take 8 x 8.4 MiB of sort and curve scratch: a chunk of 64 MiB holds 7."""
    N, S, K = 32768, 8, 32
    assert 7 * (12 * N + 8 * N * K) <= 64 << 20 < 8 * (12 * N + 8 * N * K)
    scores, ious, tp = problem(N, S, seed=11, decimals=3)
    both(scores, ious, tp, np.linspace(0.05, 0.95, K), False, 0.8, [0], [N])


def test_one_label_segments_and_equal_scores():
    N = 700
    scores, ious, tp = problem(N, 2, seed=3)
    tp[100:300], ious[100:300] = True, 0.99             # all correct
    tp[400:600] = False                                 # all wrong
    scores[1] = 0.25                                    # one column: all scores equal
    lo, hi = [100, 400, 0, 100, 399], [300, 600, N, 301, 600]
    roc, n_label, mom, removed = both(scores, ious, tp, DEFAULT6, True, 0.95, lo, hi)
    assert np.isposinf(roc[:2, ..., 0]).all() and np.isnan(roc[:2, ..., 1:]).all()
    assert (removed[:2, ..., :2] == 0).all() and (removed[0, ..., 2] == 0).all() and (removed[1, ..., 2] == 200).all()
    assert (n_label[0] == [200, 0]).all() and (n_label[1] == [0, 200]).all()
    assert (mom[0, :, :, 1] == 0).all() and (mom[1, :, :, 0] == 0).all()
    assert (mom[2:, 1, :, :, 1] == 0).all()             # equal scores: m2 is exactly 0, the mean is the score


def test_segment_order_does_not_matter():
    N = 3000
    scores, ious, tp = problem(N, 3, seed=5)
    segs = ragged_segments(N)
    perm = np.random.default_rng(1).permutation(len(segs))
    args = (scores, ious, tp, DEFAULT6, False, 0.8)
    a = TH.report_np(*args, segs[:, 0], segs[:, 1])
    b = TH.report_np(*args, segs[perm, 0], segs[perm, 1])
    for x, y in zip(a, b):
        assert x[perm].tobytes() == y.tobytes()
    # a segment's thr / rate are those of the objective on the gathered rows
    for lo, hi, r in zip(segs[:, 0], segs[:, 1], a[0]):
        if hi - lo >= 2:
            thr, rate, _ = TH.roc_objective(scores[:, lo:hi], ious[lo:hi], tp[lo:hi], DEFAULT6, np.eye(3), False, 0.8)
            assert np.array_equal(thr, r[..., 0]) and np.array_equal(rate, r[..., 1], equal_nan=True)


def test_many_segments():
    """More segments than one launch of the curve kernels per segment would make comfortable to check by eye: 1024 of them."""
    N = 2100
    scores, ious, tp = problem(N, 1, seed=9)
    rng = np.random.default_rng(2)
    lo = rng.integers(0, N - 40, 1024).astype(np.int32)
    hi = (lo + rng.integers(0, 40, 1024)).astype(np.int32)
    both(scores, ious, tp, [0.5], True, 0.95, lo, hi)


@pytest.mark.parametrize("c", H.CASES)
def test_device_reproduces_the_reference(c, tmp_path):
    g = H.gold_case(c)
    rep = TH.thr_report(H.columns(g), g["ious"], g["tp_class"], g["iou_thrs"], g["fix_cd"], g["budget"], gt_classes=g["gt_classes"])
    H.check_against_fixture(rep, g)
    label_map = None if g["gt_classes"] is None else {i + 1: "class%d" % (i + 1) for i in range(int(g["gt_classes"].max()))}
    got = TH.save_thr_performance(str(tmp_path), g["params"], list(g["uncerts"]), g["opt_uncert"], g["tp_class"], g["ious"],
                                  gt_classes=g["gt_classes"], opt_params=None if g["opt_params"] is None else list(g["opt_params"]),
                                  label_map=label_map, added_name="_" + c)
    (name,) = os.listdir(tmp_path)
    assert (tmp_path / name).read_bytes() == g["txt"]
    if g["opt_params"] is None:
        assert got == g["fprs_opt"]
    else:
        assert got[0] == g["fprs_opt"] and [[str(x) for x in row] for row in got[1]] == g["table"].tolist()
    cr, fr, frem, thr = TH.collect_thresh_results(g["opt_uncert"], g["ious"], g["tp_class"], float(g["iou_thrs"].max()),
                                                  params=g["params"])
    assert thr == g["collect_thr"] and [cr.sum(), fr.sum(), frem.sum()] == g["collect_counts"].tolist()


def test_threshold_analysis_on_the_device_equals_the_mirror(tmp_path):
    rng = np.random.default_rng(5)
    N = 300
    tp = rng.random(N) < 0.9
    ious = np.round(rng.uniform(0.3, 1.0, N), 3)
    wrong = ~(tp & (ious >= 0.5))
    good = np.round(np.where(wrong, rng.normal(0.7, 0.2, N), rng.normal(0.3, 0.2, N)).clip(0, 2), 3)
    noise = np.round(rng.uniform(0, 1, N), 3)
    gt = rng.choice([1.0, 2.0, 4.0], N)
    pred = np.where(tp, gt, rng.choice([1.0, 2.0, 4.0], N))
    params = {"thr_cd": False, "thr_fpr_tpr": 0.9, "thr_iou_thrs": [0.5, 0.75]}
    os.mkdir(tmp_path / "dev"), os.mkdir(tmp_path / "mir")
    dev = TH.threshold_analysis(str(tmp_path / "dev"), params, gt, pred, tp, ious, [good, noise], per_cls=True, population=12, rounds=2)
    mir = TH.threshold_analysis(str(tmp_path / "mir"), params, gt, pred, tp, ious, [good, noise], per_cls=True, population=12, rounds=2,
                                objective=thr_ref.roc_objective, report=RR.report_np)
    assert dev["all_opt_params"] == mir["all_opt_params"] and dev["fixed_opt_params"] == mir["fixed_opt_params"]
    assert dev["fprs_opt"] == mir["fprs_opt"]
    for name in sorted(os.listdir(tmp_path / "mir")):
        assert (tmp_path / "dev" / name).read_bytes() == (tmp_path / "mir" / name).read_bytes(), name
