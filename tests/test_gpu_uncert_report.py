"""uda_uncert_report_np on the device against the numpy mirror of its contract (tests/uncert_report_ref.py): every run goes through
the C ABI (`uncertainty_report.report_np`).

Integers are equal.  The float64 sums are the mirror's tree BIT FOR BIT (a NaN where the mirror has one): the device adds the
same terms in the same tree, every operation rounded on its own.  The one exception is S_nll, whose terms take the device's
`log`: that is not numpy's correctly-rounded-or-not `log` bit for bit, each may be off by an ulp of log(sigma) (together
4 * 2**-53 * |log sigma| a term), and trees of slightly different terms also round differently at their nodes, each within the
pairwise bound (log2(4N) + 2) * 2**-53 * sum|term|.  So S_nll is held to 2 * (log2(4N) + 2) * 2**-53 * sum|term| +
4 * 2**-53 * sum|log sigma|.

Sizes: 1 and either side of a wave (63, 64, 65), either side of the run of rows a block takes (capi.REPORT_ROWS - 1, the run,
+ 1; 255 / 256 / 257 today) and two runs + 1, where the second kernel folds three run roots padded to four."""
import os

import numpy as np
import pytest

import uncert_report_ref as R
from common import FULL_MC, make_images, make_params, make_weights
from uda_amd import capi, uncertainty_report as ur

pytestmark = pytest.mark.gpu
RUN = capi.REPORT_ROWS
SIZES = sorted({1, 63, 64, 65, 255, 256, 257, RUN - 1, RUN, RUN + 1, 2 * RUN + 1})


def make(n, K, seed, special=True):
    """n matched rows and K sigma columns; with `special`, column 0 carries sigma = 0, +inf and NaN and some rows a residual of
    0 (where n allows), and a ground-truth coordinate is 0."""
    rng = np.random.default_rng([seed, n, K])
    y1, x1 = rng.uniform(5, 300, n), rng.uniform(5, 300, n)
    gt = np.stack([y1, x1, y1 + rng.uniform(10, 200, n), x1 + rng.uniform(10, 200, n)], 1)
    pred = gt + rng.normal(0, 3, (n, 4))
    sig = rng.uniform(0.05, 8, (K, n, 4))
    gc = rng.integers(1, 4, n).astype(np.float64)
    pc = np.where(rng.uniform(size=n) < 0.2, gc + 1, gc)
    if special:
        for j, v in enumerate((0.0, np.inf, np.nan)):
            sig[0, (3 * j) % n, j] = v
        pred[n // 2] = gt[n // 2]                            # residual 0 in all four, under whatever sigma the row has
        pred[n - 1, 1] = gt[n - 1, 1]
        gt[n // 3, 0] = 0.0
        pred[(2 * n) // 3] = gt[(2 * n) // 3] + 1000.0       # IoU 0
    return gt, pred, sig, gc, pc


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(nan, 0.0, a).view(np.uint64), np.where(nan, 0.0, b).view(np.uint64))


def check(got, want, gt, pred, sig, off):
    for k in ("seg_counts", "col_counts", "ece_count"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert same_bits(got["seg_sums"], want["seg_sums"]), (got["seg_sums"], want["seg_sums"])
    assert same_bits(got["col_sums"][..., :2], want["col_sums"][..., :2]), (got["col_sums"], want["col_sums"])
    for b in range(len(off) - 1):
        n = int(off[b + 1] - off[b])
        for k in range(len(sig)):
            g, w = got["col_sums"][b, k, 2], want["col_sums"][b, k, 2]
            if n == 0:
                assert g == 0.0 and w == 0.0
                continue
            t = R.sum_abs_terms(gt[off[b]:off[b + 1]], pred[off[b]:off[b + 1]], sig[k][off[b]:off[b + 1]])
            bound = 2 * (np.log2(4 * n) + 2) * 2.0 ** -53 * t["S_nll"] + 4 * 2.0 ** -53 * t["log_sigma"]
            print("S_nll segment %d column %d: device %r mirror %r bound %g" % (b, k, g, w, bound))
            assert np.isfinite(w) and abs(g - w) <= bound, (b, k, g, w, bound)


def run_both(gt, pred, sig, gc, pc, segments=None, levels=100):
    got = ur.report_np(gt, pred, list(sig), gc, pc, segments, levels)
    want = R.report(gt, pred, sig, gc, pc, segments, levels)
    off = want["off"]
    check(got, want, gt, pred, sig, off)
    return got


@pytest.mark.parametrize("n", SIZES)
def test_sizes(n):
    got = run_both(*make(n, 3, seed=1))
    assert got["seg_counts"][0, 0] == n and got["col_counts"][0, 0, 2] == 3 and got["z"][0] == 0.0 and got["z"][-1] == -np.inf


@pytest.mark.parametrize("levels", [1, 64, 100, 128])
def test_levels_and_one_column(levels):
    got = run_both(*make(RUN + 1, 1, seed=2), levels=levels)
    assert got["ece_count"].shape == (1, 1, 4, levels) and got["z"][0] == 0.0 and (levels == 1 or got["z"][-1] == -np.inf)
    # z = 0: only a residual of 0 is inside (and not under an infinite or NaN sigma); z = -inf: every row with a usable sigma
    assert got["ece_count"][0, 0, :, 0].min() >= 1 and got["ece_count"][0, 0, :, 0].max() <= 2


def test_empty_segments():
    gt, pred, sig, gc, pc = make(RUN + 40, 3, seed=3)
    off = np.array([0, 100, 100, RUN + 40], np.int64)
    got = run_both(gt, pred, sig, gc, pc, segments=off)
    assert not got["seg_counts"][1].any() and not got["ece_count"][1].any() and not got["col_sums"][1].any() and not got["seg_sums"][1].any()
    none = run_both(np.zeros((0, 4)), np.zeros((0, 4)), np.zeros((2, 0, 4)), np.zeros(0), np.zeros(0))
    assert all(not none[k].any() for k in ("seg_counts", "col_counts", "ece_count", "seg_sums", "col_sums"))


def test_all_rows_identical():
    n = 2 * RUN + 1
    gt, pred, sig = np.tile([10.0, 20.0, 110.0, 220.0], (n, 1)), np.tile([11.0, 20.0, 108.5, 223.0], (n, 1)), np.full((2, n, 4), 1.5)
    got = run_both(gt, pred, sig, np.ones(n), np.ones(n))
    assert set(np.unique(got["ece_count"])) <= {0, n} and got["col_counts"][0, 0].tolist() == [0, 3 * n, 0]


def test_row_permutation_leaves_the_integers():
    gt, pred, sig, gc, pc = make(2 * RUN + 1, 3, seed=4)
    off = np.array([0, 70, 2 * RUN + 1], np.int64)
    a = ur.report_np(gt, pred, list(sig), gc, pc, off)
    rng = np.random.default_rng(5)
    perm = np.concatenate([rng.permutation(70), 70 + rng.permutation(2 * RUN + 1 - 70)])
    b = ur.report_np(gt[perm], pred[perm], [s[perm] for s in sig], gc[perm], pc[perm], off)
    for k in ("seg_counts", "col_counts", "ece_count"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_segment_agreement():
    """The same rows as the one segment of a call, or as the first of three, give identical outputs for that segment."""
    gt, pred, sig, gc, pc = make(2 * RUN + 60, 3, seed=6)
    n = RUN + 1
    alone = ur.report_np(gt[:n], pred[:n], [s[:n] for s in sig], gc[:n], pc[:n])
    three = ur.report_np(gt, pred, list(sig), gc, pc, np.array([0, n, n + 7, len(gt)], np.int64))
    for k in ("seg_counts", "col_counts", "ece_count"):
        np.testing.assert_array_equal(alone[k][0], three[k][0], err_msg=k)
    assert same_bits(alone["seg_sums"][0], three["seg_sums"][0]) and same_bits(alone["col_sums"][0], three["col_sums"][0])


def test_refusals_leave_the_outputs_untouched():
    lib = capi.load()
    x, c, z, s = np.ones((2, 4)), np.ones(2), np.zeros(128), np.ones((17, 2, 4))
    outs = [np.full(4096, 7, np.int64) for _ in range(3)] + [np.full(64, 7.0) for _ in range(2)]
    ok, bad0, desc, many = (np.array(o, np.int64) for o in ([0, 2], [1, 2], [0, 2, 1], [0, (1 << 22) + 1]))
    p = lambda a: None if a is None else a.ctypes.data                         # noqa: E731

    def call(B=1, K=1, L=100, off=ok, gt=x, zz=z):
        return lib.uda_uncert_report_np(0, B, K, L, p(off), p(gt), p(x), p(c), p(c), p(s), p(zz), *[o.ctypes.data for o in outs])
    for kw, word in ((dict(B=0), "segments"), (dict(K=0), "sigma columns"), (dict(K=17), "sigma columns"), (dict(L=0), "levels"),
                     (dict(L=129), "levels"), (dict(off=None), "NULL"), (dict(zz=None), "NULL"), (dict(off=bad0), "not at 0"),
                     (dict(B=2, off=desc), "do not ascend"), (dict(off=many), "at most"), (dict(gt=None), "NULL input")):
        assert call(**kw) == 1, kw
        msg = lib.uda_last_error(None).decode()
        assert msg.startswith("uda_uncert_report_np: ") and word in msg, (kw, msg)
        assert all((o == 7).all() for o in outs), kw
    assert call() == 0 and outs[0][0] == 2 and not (outs[2][:400] == 7).any()


def test_driver_path_writes_the_reference_lines(tmp_path):
    """A tiny synthetic model with MC dropout and loss attenuation through validate_to_file(..., uncert_report=True): the lines
    appended to model_performance.txt are those `uncertainty_report` gives for the returned matched rows through the mirror -
    the ECE lines and the counts' lines as characters, mIoU and RMSE bit for bit too (the device's sums are the mirror's)."""
    from uda_amd import writers
    from uda_amd.infer_lib import KerasDriver
    p = make_params(image_size="256x128", **FULL_MC)
    d = KerasDriver("_", False, p["name"], 2, False, p, weights=make_weights(p, seed=12, cls_spread=20.0))
    try:
        d.set_dropout_seed(23)
        batch = make_images(2, 140, 260, seed=11)
        det = d.serve(batch)
        rng = np.random.default_rng(8)
        G = 6
        gb, gc = np.full((2, G, 4), -1, np.float32), np.full((2, G), -1, np.float32)
        for i in range(2):
            ranks = rng.integers(0, max(int(det[3][i]), 1), 4)
            gb[i, :4] = det[0][i, ranks, :4] + rng.normal(0, 0.5, (4, 4)).astype(np.float32)
            gb[i, 4] = [5000, 5000, 5100, 5200]                                 # matches nothing: IoU 0
            gc[i, :5] = rng.integers(1, 8, 5)
        out = str(tmp_path / "plain")
        plain = writers.validate_to_file(d, [batch], [(gb, gc)], [["a.png", "b.png"]], out)
        assert "uncert_report" not in plain and not os.path.exists(os.path.join(out, "model_performance.txt"))
        out = str(tmp_path / "report")
        f = writers.validate_to_file(d, [batch], [(gb, gc)], [["a.png", "b.png"]], out, uncert_report=True)
        rep = f["uncert_report"]
        assert rep.names == ["albox", "mcbox"] and rep.count("n_rows") == len(f["names"]) == 10 and rep.count("n_iou_zero") >= 2
        want = ur.from_filtered(f, engine=R.report)
        dec = p["uncert_adjust_method"]
        lines = ur.model_performance_lines(want, "aleatoric", dec) + ur.model_performance_lines(want, "mcdropout", dec, exists=True)
        text = open(os.path.join(out, "model_performance.txt")).read()
        assert text == "".join(lines) and len(lines) == 7 and text.count(" \n") == 7
        assert lines[5].startswith("ECE Loc aleatoric: ") and lines[6].startswith("ECE mcdropout: ")
        for k in ("seg_counts", "col_counts", "ece_count"):
            np.testing.assert_array_equal(getattr(rep, k), getattr(want, k), err_msg=k)
    finally:
        d.close()
