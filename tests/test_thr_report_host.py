"""The thresholding report, host side (`uda_amd.thresholding`: calc_jsd, thr_report, save_thr_performance, collect_thresh_results,
the `_clsoptfix` rule, threshold_analysis; reference uncertainty_analysis.py:398-500, :517-749, utils_extra.py:25-36): the numpy
mirror (tests/thr_report_ref.py) against what the reference's own functions returned (tests/golden/thr_report_golden.npz), the
texts and tables byte for byte with the mirror standing in for the device, and the refusals.

Bounds.  thr, rate and every count are exact.  auc: N * 2^-52.  The moments differ from numpy's only by the
order of summation (the stated tree against numpy's pairwise sum); measured on this fixture, mirror against np.mean / np.std /
calc_jsd: mean 5.4e-16, std 2.7e-16, JSD 2.3e-15, all relative.  The tests allow 16 times those figures."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import thr_ref
import thr_report_ref as RR
from uda_amd import capi
from uda_amd import thresholding as TH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "thr_report_golden.npz"))
CASES = [str(c) for c in GOLD["cases"]]
MEAN_BOUND, STD_BOUND, JSD_BOUND = 16 * 5.4e-16, 16 * 2.7e-16, 16 * 2.3e-15


def gold_case(c):
    g = {k: GOLD["%s_%s" % (c, k)] for k in ("uncerts", "opt_uncert", "ious", "tp_class", "iou_thrs", "roc", "jsd", "mean", "std",
                                             "n_label", "collect_counts")}
    g["fix_cd"], g["budget"], g["fprs_opt"] = int(GOLD[c + "_fix_cd"]), float(GOLD[c + "_budget"]), float(GOLD[c + "_fprs_opt"])
    g["collect_thr"] = float(GOLD[c + "_collect_thr"])
    g["txt"] = bytes(GOLD[c + "_txt"])
    for k in ("gt_classes", "opt_params", "table"):
        g[k] = GOLD["%s_%s" % (c, k)] if "%s_%s" % (c, k) in GOLD.files else None
    g["params"] = {"thr_cd": bool(g["fix_cd"]), "thr_fpr_tpr": g["budget"], "thr_iou_thrs": [float(t) for t in g["iou_thrs"]]}
    return g


def columns(g):
    """The score columns of the fixture's raw arrays: the uncertainties, opt_uncert, and with opt_params the per-class column."""
    cols = list(g["uncerts"]) + [g["opt_uncert"]]
    if g["opt_params"] is not None:
        U, gt, col, n_iter = len(g["uncerts"]), g["gt_classes"], np.zeros(g["opt_uncert"].size), 0
        for i in range(int(gt.max())):
            sel = np.where(gt == i + 1)[0]
            if len(sel) == 0:
                continue
            if len(g["opt_params"]) == U:
                col[sel] = sum(p * u[sel] for p, u in zip(g["opt_params"], g["uncerts"]))
            else:
                col[sel] = np.sum([u[sel] * g["opt_params"][n_iter + j] for j, u in enumerate(g["uncerts"])], axis=0)
                n_iter += U
        cols.append(col)
    return np.stack(cols)


def check_against_fixture(rep, g):
    """A ThrReport of columns(g) over all rows and the classes, against the reference's raw values."""
    N = g["uncerts"].shape[1]
    assert np.array_equal(rep.thr, g["roc"][..., 0])
    assert np.array_equal(rep.rate, g["roc"][..., 1], equal_nan=True)
    ref_auc = g["roc"][..., 2]
    assert np.array_equal(np.isnan(rep.auc), np.isnan(ref_auc))
    ok = ~np.isnan(ref_auc)
    assert (np.abs(rep.auc[ok] - ref_auc[ok]) <= N * 2.0 ** -52).all()
    assert np.array_equal(rep.n_correct, g["n_label"][..., 0]) and np.array_equal(rep.n_wrong, g["n_label"][..., 1])
    assert np.array_equal(np.isnan(rep.mean), np.isnan(g["mean"]))
    ok = ~np.isnan(g["mean"])
    err_m = np.max(np.abs(rep.mean[ok] - g["mean"][ok]) / np.abs(g["mean"][ok]).clip(1e-300))
    assert np.array_equal(rep.std[ok] == 0, g["std"][ok] == 0)      # a zero std decides between NaN and a number downstream
    pos = ok & (g["std"] > 0)
    err_s = np.max(np.abs(rep.std[pos] - g["std"][pos]) / g["std"][pos], initial=0.0)
    jsd, ref = rep.jsd, np.nan_to_num(g["jsd"])
    assert np.array_equal(jsd == 0, ref == 0)
    nz = ref != 0
    err_j = np.max(np.abs(jsd[nz] - ref[nz]) / ref[nz], initial=0.0)
    print("relative errors: mean %.3g  std %.3g  jsd %.3g" % (err_m, err_s, err_j))
    assert err_m <= MEAN_BOUND and err_s <= STD_BOUND and err_j <= JSD_BOUND


def test_fixture_covers_what_it_should():
    gs = {c: gold_case(c) for c in CASES}
    assert {g["uncerts"].shape[1] for g in gs.values()} >= {2, 3, 65, 257, 1025, 3000}
    assert {g["uncerts"].shape[0] for g in gs.values()} == {1, 2, 3} and {g["iou_thrs"].size for g in gs.values()} == {1, 2, 6}
    assert {(g["fix_cd"], g["budget"]) for g in gs.values()} == {(0, 0.8), (0, 0.95), (1, 0.8), (1, 0.95)}
    kinds = set()
    for g in gs.values():
        if g["opt_params"] is None:
            continue
        U, gt = g["uncerts"].shape[0], g["gt_classes"]
        C = int(gt.max())
        kinds.add("global" if len(g["opt_params"]) == U else "percls")
        assert any(not (gt == c).any() and (gt < c).any() for c in range(1, C)), "an empty class in the middle"
    assert kinds == {"global", "percls"}
    big = gs["n3000_cd_global"]["gt_classes"]
    assert 2048 < (big == 1).sum() < 3000
    g = gs["n257_u3_percls"]
    gt, correct = g["gt_classes"], (g["ious"] >= 0.5) & (g["tp_class"] != 0)
    assert (gt == 2).sum() == 1 and (gt == 3).sum() == 2 and correct[gt == 5].all() and (gt == 5).sum() > 2
    two = np.flatnonzero(gt == 3)
    assert (g["uncerts"][:, two[0]] == g["uncerts"][:, two[1]]).all() and correct[two].sum() == 1
    assert np.isnan(g["jsd"][3]).all() and (g["std"][3] == 0).all()            # std 0 -> NaN -> 0
    assert np.isposinf(g["roc"][5, ..., 0]).all() and np.isnan(g["roc"][5, ..., 1]).all()
    ties = gs["n1025_ties"]
    assert len(np.unique(ties["opt_uncert"])) < 128


@pytest.mark.parametrize("c", CASES)
def test_mirror_reproduces_the_reference(c):
    g = gold_case(c)
    rep = TH.thr_report(columns(g), g["ious"], g["tp_class"], g["iou_thrs"], g["fix_cd"], g["budget"], gt_classes=g["gt_classes"],
                        report=RR.report_np)
    check_against_fixture(rep, g)
    # a segment's thr / rate are those of the objective's mirror on the gathered rows; counts are numpy compares against thr
    cols = columns(g)[:, rep.order]
    ious, tp = g["ious"][rep.order], g["tp_class"][rep.order]
    for b in range(len(rep.seg_lo)):
        sl = slice(rep.seg_lo[b], rep.seg_hi[b])
        assert np.array_equal(rep.n_correct[b] + rep.n_wrong[b], np.full(g["iou_thrs"].size, sl.stop - sl.start))
        if sl.stop - sl.start >= 2:
            thr, rate, _ = thr_ref.roc_objective(cols[:, sl], ious[sl], tp[sl], g["iou_thrs"], np.eye(len(cols)), g["fix_cd"],
                                                 g["budget"])
            assert np.array_equal(thr, rep.thr[b]) and np.array_equal(rate, rep.rate[b], equal_nan=True)
        for k, t in enumerate(g["iou_thrs"]):
            correct = (ious[sl] >= t) & (tp[sl] != 0)
            for s in range(len(cols)):
                rem = cols[s, sl] >= rep.thr[b, s, k]
                assert (rep.correctly_removed[b, s, k], rep.falsely_removed[b, s, k], rep.falsely_remaining[b, s, k]) == \
                    ((rem & ~correct).sum(), (rem & correct).sum(), (~rem & ~correct).sum())
                if np.isposinf(rep.thr[b, s, k]):
                    assert rep.correctly_removed[b, s, k] == 0 and rep.falsely_removed[b, s, k] == 0


@pytest.mark.parametrize("c", CASES)
def test_texts_and_tables_byte_for_byte(c, tmp_path):
    g = gold_case(c)
    label_map = None if g["gt_classes"] is None else {i + 1: "class%d" % (i + 1) for i in range(int(g["gt_classes"].max()))}
    got = TH.save_thr_performance(str(tmp_path), g["params"], list(g["uncerts"]), g["opt_uncert"], g["tp_class"], g["ious"],
                                  gt_classes=g["gt_classes"], opt_params=None if g["opt_params"] is None else list(g["opt_params"]),
                                  label_map=label_map, added_name="_" + c, report=RR.report_np)
    name = "thr_metrics_%s_%s_iou_%s_%s_%s.txt" % ("cd" if g["fix_cd"] else "fd", g["budget"], g["iou_thrs"].min(),
                                                   g["iou_thrs"].max(), c)
    assert os.listdir(tmp_path) == [name]
    assert (tmp_path / name).read_bytes() == g["txt"]
    if g["opt_params"] is None:
        assert got == g["fprs_opt"]
    else:
        fprs_opt, table = got
        assert fprs_opt == g["fprs_opt"]
        assert [[str(x) for x in row] for row in table] == g["table"].tolist()
    # the mirror's own text from its raw values
    U = g["uncerts"].shape[0]
    rep = TH.thr_report(columns(g)[:U + 1], g["ious"], g["tp_class"], g["iou_thrs"], g["fix_cd"], g["budget"], report=RR.report_np)
    metric = ("FD@CD" if g["fix_cd"] else "CD@FD") + str(int(g["budget"] * 100))
    assert RR.metrics_text(rep.jsd[0], rep.auc100[0], rep.fdcd[0], metric).encode() == g["txt"]


def test_calc_jsd_is_the_references():
    g = gold_case("n257_u3_percls")
    cols, gt = columns(g), g["gt_classes"]
    segs = [np.arange(gt.size)] + [np.flatnonzero(gt == c + 1) for c in range(int(gt.max()))]
    seen_nan = seen = 0
    for b, sel in enumerate(segs):
        for k, t in enumerate(g["iou_thrs"]):
            correct = (g["ious"][sel] >= t) & (g["tp_class"][sel] != 0)
            for s in range(len(cols)):
                u = cols[s][sel]
                got = TH.calc_jsd(u[correct], u[~correct]) if len(sel) else np.nan
                assert np.array_equal(got, g["jsd"][b, s, k], equal_nan=True), (b, s, k)       # the same expression: the same bits
                seen_nan += bool(np.isnan(got))
                seen += 1
    assert 0 < seen_nan < seen
    assert np.isnan(TH.calc_jsd(np.array([]), np.array([1.0, 2.0]))) and np.isnan(TH.calc_jsd(np.array([0.5, 0.5]), np.array([1.0, 2.0])))
    assert np.isnan(TH.jsd_from_moments(np.nan, np.nan, 1.0, 0.2)) and np.isnan(TH.jsd_from_moments(0.4, 0.0, 1.0, 0.2))
    assert TH.jsd_from_moments(0.4, 0.1, 0.4, 0.1) == 0.0 and 0 < TH.jsd_from_moments(0.4, 0.1, 1.0, 0.2) < 1


def test_segments_by_class_orders_stably():
    gt = np.array([3, 1, 5, 3, 1, 1, 5, 3.0])
    order, lo, hi = TH.segments_by_class(gt, 6)
    assert order.tolist() == [1, 4, 5, 0, 3, 7, 2, 6]
    assert lo.tolist() == [0, 0, 3, 3, 6, 6, 8] and hi.tolist() == [8, 3, 3, 6, 6, 8, 8]
    assert lo.dtype == hi.dtype == np.int32
    order, lo, hi = TH.segments_by_class(gt)
    assert len(lo) == 6 and hi[-1] == 8
    for bad in ([0.0, 1.0], [1.5, 2.0], []):
        with pytest.raises(ValueError):
            TH.segments_by_class(np.asarray(bad))
    with pytest.raises(ValueError):
        TH.segments_by_class(gt, 4)


def test_clsoptfix_rule():
    glob, perc = [0.5, 0.25], [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0]
    #            worse      equal      exactly 100    better     no rows
    all_fdcd = [40.0, 40.0, 100.0, 40.0, 0.0]
    cur_fdcd = [39.999, 40.0, 100.0, 40.001, 0.0]
    fixed = TH.clsoptfix_params(glob, perc, all_fdcd, cur_fdcd, has_rows=[True, True, True, True, False])
    assert fixed == [0.5, 0.25, 0.3, 0.4, 0.5, 0.25, 0.7, 0.8, 0.9, 1.0]
    assert perc[0] == 0.1                                           # the input list is left alone
    assert TH.clsoptfix_params(glob, perc, all_fdcd, cur_fdcd)[8:] == [0.9, 1.0]          # 0 < 0 is false, 0 != 100


def test_odd_k_raises_with_a_table_and_works_without(tmp_path):
    g = gold_case("n65_u1_global")
    params = dict(g["params"], thr_iou_thrs=[0.5, 0.6, 0.7])
    args = (str(tmp_path), params, list(g["uncerts"]), g["opt_uncert"], g["tp_class"], g["ious"])
    with pytest.raises(ValueError, match="odd"):
        TH.save_thr_performance(*args, gt_classes=g["gt_classes"], opt_params=list(g["opt_params"]), report=RR.report_np)
    assert os.listdir(tmp_path) == []
    assert np.isfinite(TH.save_thr_performance(*args, report=RR.report_np))
    assert len(os.listdir(tmp_path)) == 1
    with pytest.raises(ValueError, match="gt_classes"):
        TH.save_thr_performance(*args, opt_params=list(g["opt_params"]), report=RR.report_np)


@pytest.mark.parametrize("c", ["n65_u1_global", "n3000_fd_percls", "n2_txt"])
def test_collect_thresh_results(c):
    g = gold_case(c)
    t = float(g["iou_thrs"].max())
    cr, fr, frem, thr = TH.collect_thresh_results(g["opt_uncert"], g["ious"], g["tp_class"], t, params=g["params"], report=RR.report_np)
    assert thr == g["collect_thr"]
    assert [cr.sum(), fr.sum(), frem.sum()] == g["collect_counts"].tolist()
    assert cr.dtype == bool and not (cr & fr).any() and not (cr & frem).any()


def test_threshold_analysis_runs_the_references_sequence(tmp_path):
    rng = np.random.default_rng(5)
    N = 300
    tp = rng.random(N) < 0.9
    ious = np.round(rng.uniform(0.3, 1.0, N), 3)
    wrong = ~(tp & (ious >= 0.5))
    good = np.round(np.where(wrong, rng.normal(0.7, 0.2, N), rng.normal(0.3, 0.2, N)).clip(0, 2), 3)
    noise = np.round(rng.uniform(0, 1, N), 3)
    gt = rng.choice([1.0, 2.0, 4.0], N)                             # class 3 has no row
    pred = np.where(tp, gt, rng.choice([1.0, 2.0, 4.0], N))
    params = {"thr_cd": True, "thr_fpr_tpr": 0.9, "thr_iou_thrs": [0.5, 0.75]}
    out = TH.threshold_analysis(str(tmp_path), params, gt, pred, tp, ious, [good, noise], per_cls=True, objective=thr_ref.roc_objective,
                                report=RR.report_np, population=12, rounds=2)
    tail = "cd_0.9_iou_0.5_0.75"
    assert sorted(os.listdir(tmp_path)) == sorted(
        ["optimal_params_%s.txt" % tail, "optimal_thrs_%s.txt" % tail, "optimal_params_%s_clsopt.txt" % tail,
         "optimal_thrs_%s_clsopt.txt" % tail] + ["thr_metrics_%s%s.txt" % (tail, a) for a in ("", "_clsoptpred", "_clsopt", "_clsoptfix")])
    assert len(out["all_opt_params"]) == 2 and len(out["perc_opt_params"]) == 8 and len(out["fixed_opt_params"]) == 8
    has = [True, True, False, True]
    assert out["fixed_opt_params"] == TH.clsoptfix_params(out["all_opt_params"], out["perc_opt_params"], out["all_fdcd"],
                                                          out["current_fdcd"], has)
    assert out["fixed_opt_params"][4:6] == out["perc_opt_params"][4:6]          # the class without rows keeps its weights
    # per class, the rule's two figures are what save_thr_performance returns on that class's rows alone
    for c in (1, 2, 4):
        sel = gt == c
        per = [good[sel], noise[sel]]
        for key, w in (("all_fdcd", out["all_opt_params"]), ("current_fdcd", out["perc_opt_params"][2 * (c - 1):2 * c])):
            f = TH.save_thr_performance(str(tmp_path), params, per, sum(p * u for p, u in zip(w, per)), tp[sel], ious[sel],
                                        added_name="_probe", report=RR.report_np)
            assert f == out[key][c - 1]
    assert set(out["tables"]) == {"", "_clsopt", "_clsoptfix"} and set(out["fprs_opt"]) == {"", "_clsoptpred", "_clsopt", "_clsoptfix"}
    assert [r[0] for r in out["tables"][""]] == ["Classes", "IoU Thr.", "1", "2", "3", "4", "Avg. perc", "Orig. U.0", "Orig. U.1", "Opt. Combo"]
    assert [str(x) for x in out["tables"]["_clsopt"][4][1:]] == ["0.0"] * 9         # the class without rows: zeros


# ------------------------------------------------------------------ refusals
def small():
    return dict(scores=np.array([[0.1, 0.9, 0.5, 0.3]]), ious=np.array([0.9, 0.9, 0.2, 0.8]), tp_class=np.array([1, 1, 1, 0]),
                iou_thrs=[0.5], fix_cd=True, budget=0.95, seg_lo=[0], seg_hi=[4])


@pytest.mark.parametrize("change, match", [
    (dict(scores=np.zeros((9, 4))), "score columns"), (dict(scores=np.zeros((1, 1)), ious=[0.5], tp_class=[1], seg_hi=[1]), "rows"),
    (dict(ious=np.zeros(3)), "ious of 3"), (dict(iou_thrs=np.linspace(0.1, 0.9, 33)), "IoU thresholds"), (dict(iou_thrs=[]), "IoU thresholds"),
    (dict(budget=0.0), "budget"), (dict(budget=1.0), "budget"), (dict(seg_lo=[-1]), "segment"), (dict(seg_hi=[5]), "segment"),
    (dict(seg_lo=[3], seg_hi=[2]), "segment"), (dict(seg_lo=[0, 1]), "segment bounds"), (dict(seg_lo=[], seg_hi=[]), "segment bounds"),
    (dict(scores=np.array([[0.1, np.nan, 0.5, 0.3]])), "NaN or inf"), (dict(ious=np.array([0.9, np.inf, 0.2, 0.8])), "NaN or inf"),
])
def test_python_refusals(change, match):
    a = dict(small(), **change)
    with pytest.raises(ValueError, match=match):
        TH.report_np(**a)


def test_library_refusals_leave_the_outputs_untouched():
    lib = capi.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)        # noqa: E731
    sc, io, tp, th = np.ones((1, 4)), np.ones(4), np.ones(4, np.uint8), np.array([0.5])
    lo, hi = np.zeros(1, np.int32), np.full(1, 4, np.int32)
    roc, nl, mom, rem = np.full((1, 1, 1, 3), 7.0), np.full((1, 1, 2), 7, np.int64), np.full((1, 1, 1, 2, 2), 7.0), np.full((1, 1, 1, 3), 7, np.int64)

    def call(N=4, S=1, K=1, B=1, budget=0.95, lo=lo, hi=hi, sc=sc):
        return lib.uda_thr_report_np(0, p(sc) if sc is not None else None, p(io), p(tp), N, S, p(th), K, p(lo), p(hi), B, 1, budget,
                                     p(roc), p(nl), p(mom), p(rem))
    bad = [dict(N=1), dict(N=capi.THR_MAX_N + 1), dict(S=0), dict(S=capi.THR_REPORT_MAX_S + 1), dict(K=0), dict(K=33), dict(B=0),
           dict(B=capi.THR_REPORT_MAX_SEGS + 1), dict(budget=0.0), dict(budget=1.0), dict(budget=float("nan")), dict(sc=None),
           dict(lo=np.full(1, -1, np.int32)), dict(hi=np.full(1, 5, np.int32)), dict(lo=np.full(1, 3, np.int32), hi=np.full(1, 2, np.int32))]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert lib.uda_last_error(None).decode().startswith("uda_thr_report_np: "), kw
    assert (roc == 7).all() and (nl == 7).all() and (mom == 7).all() and (rem == 7).all()
    assert capi.THR_REPORT_MAX_SEGS >= 1024


def test_symbol_is_exported_and_the_call_fails_loudly_without_a_gpu():
    assert "uda_thr_report_np" in capi.EXPORTS
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "uda_thr_report_np")
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np\n"
            "import conftest\n"
            "from uda_amd import capi, thresholding as TH\n"
            "try:\n"
            "    TH.report_np(np.array([[0.1, 0.9, 0.5, 0.3]]), [0.9, 0.9, 0.2, 0.8], [1, 1, 1, 0], [0.5], True, 0.95, [0], [4])\n"
            "    print('no error')\n"
            "except capi.UdaError as e:\n"
            "    print('UdaError|%%s' %% e)\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("UdaError|") and "uda_thr_report_np" in out.stdout and "no ROCm-capable device" in out.stdout, out.stdout
