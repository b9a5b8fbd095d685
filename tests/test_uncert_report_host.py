"""The validation uncertainty report on the host (`uncertainty_report`; reference src/utils_extra.py:378-445,
calibrate_regression.py:46-61 and 231-349, utils_box.py:17-102) without a GPU: the numpy mirror of the contract
(tests/uncert_report_ref.py) against what the reference's own functions gave (tests/golden/uncert_report_golden.npz, maker beside
it), then `UncertReport`, the per-class and the relative form, `merge` and the two texts on mirror output (`engine=`).

Counts, coverage and every ECE are equal.  A float64 sum of the mirror's tree and the reference's numpy sum are two pairwise
summations of the same 4N (or N) terms, each within (log2(4N) + 2) * 2**-53 * sum|term| of the exact sum, so they differ by at
most BOUND = 2 * (log2(4N) + 2) * 2**-53 * sum|term|.  A mean adds one rounding on either side (2**-52 relative); a root halves
the relative error of its argument and adds one rounding on either side.  The reference's sharpness squares and sums in float32:
the same with 2**-24.

The texts are compared character for character, with one exception that the bound itself forces: model_performance.txt prints
mIoU and RMSE with all their digits (`str` of a float64), and two summation orders may differ in the last of them.  On those two
lines the words, the spacing and the line end are compared as characters and the number within its bound above."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import uncert_report_ref as R
from common import ROOT
from uda_amd import capi, uncertainty_report as ur, writers

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uncert_report_golden.npz"))
CASES = ("n1", "n5", "n300")
NAMES = ("albox", "mcbox")


def inputs(case, rows=None):
    a = [GOLD["%s_%s" % (case, k)] for k in ("gt", "pred", "sigma", "gt_classes", "classes")]
    if rows is not None:
        a = [a[0][rows], a[1][rows], a[2][:, rows], a[3][rows], a[4][rows]]
    return a[0], a[1], dict(zip(NAMES, a[2])), a[3], a[4]


def rel(n_terms, eps=2.0 ** -53):
    """BOUND / sum|term| for a sum of n_terms terms."""
    return 2 * (np.log2(n_terms) + 2) * eps


def check_against_golden(rep, segment, prefix, gt, pred, sig):
    """Every number of one segment of `rep` against the golden arrays `prefix`_*; gt, pred, sig: that segment's rows."""
    n = len(gt)
    g = lambda k: GOLD[prefix + "_" + k]                                       # noqa: E731
    assert rep.count("n_rows", segment) == n
    assert rep.count("n_iou_zero", segment) == np.count_nonzero(g("ious") == 0)
    assert rep.missing_pct(segment) == float(g("md")) and rep.misclassification(segment) == float(g("misc"))
    assert abs(rep.miou(segment) - g("miou")) <= rel(n) * np.abs(g("ious")).sum() / n + 2.0 ** -52 * g("miou")
    assert abs(rep.rmse(segment) - g("rmse")) <= (rel(4 * n) / 2 + 2.0 ** -51) * g("rmse")
    for k, name in enumerate(NAMES):
        c = lambda key: GOLD["%s_c%d_%s" % (prefix, k, key)]                    # noqa: E731
        t = R.sum_abs_terms(gt, pred, sig[name])
        assert rep.count("covered_all", segment, name) == int(c("covered"))
        assert rep.ece(name, segment) == c("ece_flat") and rep.ece_box(name, segment) == c("ece_box")
        assert np.array_equal(rep.ece_per_coordinate(name, segment), c("ece_coord"))
        n_ok = 4 * n - rep.count("n_degenerate", segment, name)
        assert abs(rep.nll(name, segment) - c("nll")) <= rel(4 * n) * t["S_nll"] / n_ok + 2.0 ** -52 * abs(c("nll")), (prefix, name)
        assert abs(rep.rmsue(name, segment) - c("rmsue")) <= (rel(4 * n) / 2 + 2.0 ** -51) * c("rmsue")
        assert abs(np.float64(rep.sharpness(name, segment)) - np.float64(c("sharp"))) <= (rel(4 * n, 2.0 ** -24) / 2 + 2.0 ** -23) * c("sharp")


@pytest.mark.parametrize("case", CASES)
def test_mirror_reproduces_the_reference(case):
    gt, pred, sig, gc, pc = inputs(case)
    rep = ur.report(gt, pred, sig, gc, pc, engine=R.report)
    assert rep.names == list(NAMES) and len(rep) == 1
    check_against_golden(rep, 0, case, gt, pred, sig)


def test_levels_are_the_reference_s():
    p_m, z = ur.levels_z(100)
    assert np.array_equal(z.view(np.uint64), GOLD["z"].view(np.uint64)) and z[0] == 0.0 and z[99] == -np.inf
    assert np.array_equal(p_m, np.linspace(0, 1, 100))


def test_planted_rows_of_n5():
    gt, pred, sig, gc, pc = inputs("n5")
    rep = ur.report(gt, pred, sig, gc, pc, engine=R.report)
    assert rep.count("n_degenerate", column="albox") == 8 and rep.count("n_degenerate", column="mcbox") == 0
    assert rep.count("n_res_nonzero", column="albox") == 12 and rep.count("n_gt_nonzero") == 19 and rep.count("n_iou_zero") == 1
    # sigma = 0: level 0 (z = 0) is `|res| <= 0`, level 99 (z = -inf) is a comparison with NaN - false even for a residual of 0
    counts = rep.ece_count[0, 0]
    assert counts[:, 99].tolist() == [3, 3, 3, 3] and counts[:, 0].tolist() == [2, 2, 2, 2]
    assert np.isfinite(rep.nll("albox"))                     # (its value against the reference's: test_mirror_reproduces_the_reference)


def test_tree_does_not_depend_on_the_run_length():
    x = np.random.default_rng(3).normal(0, 1e3, 1000) ** 3
    want = R.tree(x)
    for run in (1, 2, 64, 256, 512, 1024):
        roots = [R.tree(x[i:i + run]) for i in range(0, len(x), run)]
        assert R.tree(roots) == want
    assert R.tree([]) == 0.0 and R.tree([5.0]) == 5.0


def test_the_mirrors_share_one_statement_of_the_tree():
    import class_report_ref
    import thr_report_ref
    import tree_ref
    assert R.tree is tree_ref.tree and class_report_ref.tree is tree_ref.tree and thr_report_ref.tree_sum is tree_ref.tree


def test_per_class_segments():
    gt, pred, sig, gc, pc = inputs("n300")
    ids = [float(c) for c in GOLD["class_ids"]]
    rep = ur.per_class(gt, pred, sig, gc, pc, ids, engine=R.report)
    assert rep.labels == ids and len(rep) == 3 and rep.count("n_rows", 1) == 0
    assert np.isnan(rep.miou(1)) and np.isnan(rep.ece("albox", 1)) and not rep.ece_count[1].any() and not rep.col_sums[1].any()
    for seg, c in ((0, 1), (2, 3)):
        m = gc == c
        check_against_golden(rep, seg, "n300_cls%d" % c, gt[m], pred[m], {k: v[m] for k, v in sig.items()})
    whole = ur.report(gt, pred, sig, gc, pc, engine=R.report)
    assert np.array_equal(rep.ece_count.sum(axis=0), whole.ece_count[0]) and np.array_equal(rep.seg_counts.sum(axis=0), whole.seg_counts[0])


@pytest.mark.parametrize("case", CASES)
def test_relative_ece(case):
    gt, pred, sig, _, _ = inputs(case)
    scale = np.stack([pred[:, 2] - pred[:, 0], pred[:, 3] - pred[:, 1]] * 2, 1)
    res, nsig = np.abs(gt - pred) / scale, {k: v / scale for k, v in sig.items()}
    with np.errstate(all="ignore"):
        box = ur.relative_ece(res, nsig, engine=R.report)
        one = ur.relative_ece(res[:, 0], {k: v[:, 0] for k, v in nsig.items()}, engine=R.report)
    for k, name in enumerate(NAMES):
        assert box[name] == GOLD["%s_c%d_rel_ece_box" % (case, k)] and one[name] == GOLD["%s_c%d_rel_ece_coord0" % (case, k)]
    with pytest.raises(ValueError, match="negative"):
        ur.relative_ece(-np.ones((2, 4)), [np.ones((2, 4))], engine=R.report)


def assert_same_text(text, want, tol):
    """Character for character; on a line whose label is in `tol` the number may differ by tol[label] (relative)."""
    got_lines, want_lines = text.splitlines(True), want.splitlines(True)
    assert len(got_lines) == len(want_lines), (text, want)
    for a, b in zip(got_lines, want_lines):
        label = b.split(": ")[0]
        if label in tol and a != b:
            ma, mb = (re.fullmatch(re.escape(label) + r": (\S+) \n", x) for x in (a, b))
            assert ma and mb and len(ma.group(1)) >= len(mb.group(1)) - 1, (a, b)
            assert abs(float(ma.group(1)) - float(mb.group(1))) <= tol[label] * abs(float(mb.group(1))), (a, b)
        else:
            assert a == b


@pytest.mark.parametrize("case", CASES)
def test_text_lines(case):
    gt, pred, sig, gc, pc = inputs(case)
    rep = ur.report(gt, pred, sig, gc, pc, engine=R.report)
    dec, method = str(GOLD["decoding"][0]), str(GOLD["method"][0])
    text = "".join(ur.model_performance_lines(rep, "aleatoric", dec) + ur.model_performance_lines(rep, "mcdropout", dec, exists=True))
    n = len(gt)
    assert_same_text(text, str(GOLD[case + "_model_performance"][0]), {"mIoU": rel(n) + 2.0 ** -52, "RMSE": rel(4 * n) / 2 + 2.0 ** -51})
    if case != "n5":
        text = "".join(ur.regression_logging_lines(rep, method, False, "albox") + ur.regression_logging_lines(rep, method, True, "mcbox"))
        assert text == str(GOLD[case + "_regression_logging"][0])


def test_merge():
    gt, pred, sig, gc, pc = inputs("n300")
    whole = ur.report(gt, pred, sig, gc, pc, engine=R.report)
    for cut, exact in ((256, True), (100, False)):
        a, b = (ur.report(*inputs("n300", rows), engine=R.report) for rows in (slice(0, cut), slice(cut, 300)))
        m = a.merge(b)
        for k in ("seg_counts", "col_counts", "ece_count"):
            assert np.array_equal(getattr(m, k), getattr(whole, k))
        assert m.ece("mcbox") == whole.ece("mcbox") and m.coverage_pct("albox") == whole.coverage_pct("albox")
        if exact:                                            # 256 rows, then 44: the whole's tree has exactly these two subtrees
            assert np.array_equal(m.seg_sums, whole.seg_sums) and np.array_equal(m.col_sums, whole.col_sums)
        else:
            t = R.sum_abs_terms(gt, pred, sig["albox"])
            for j, name in enumerate(ur.COL_SUMS):
                assert abs(m.col_sums[0, 0, j] - whole.col_sums[0, 0, j]) <= rel(1200) * t[name]
    with pytest.raises(ValueError, match="same columns"):
        whole.merge(ur.report(gt, pred, [sig["albox"]], gc, pc, engine=R.report))


def test_inputs_are_checked_before_the_library():
    gt, pred, sig, gc, pc = inputs("n5")
    with pytest.raises(ValueError, match="sigma column 0 has shape"):
        ur.report_np(gt, pred, [sig["albox"][:3]], gc, pc)
    with pytest.raises(ValueError, match="1..16"):
        ur.report_np(gt, pred, [sig["albox"]] * 17, gc, pc)
    with pytest.raises(ValueError, match="segments must ascend"):
        ur.report_np(gt, pred, [sig["albox"]], gc, pc, segments=[0, 3, 2, 5])
    with pytest.raises(ValueError, match="levels"):
        ur.report_np(gt, pred, [sig["albox"]], gc, pc, levels=129)


def test_binding_and_limits_match_the_header():
    text = open(capi.HEADER).read()
    for name, value in (("UDA_REPORT_ROWS", capi.REPORT_ROWS), ("UDA_REPORT_MAX_K", capi.REPORT_MAX_K), ("UDA_REPORT_MAX_L", capi.REPORT_MAX_L),
                        ("UDA_REPORT_MAX_B", capi.REPORT_MAX_B), ("UDA_REPORT_MAX_ROWS", capi.REPORT_MAX_ROWS)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value
    assert "uda_uncert_report_np" in capi.EXPORTS and len(capi._SIGNATURES["uda_uncert_report_np"][1]) == 16
    assert capi.REPORT_ROWS & (capi.REPORT_ROWS - 1) == 0    # a run is a power of two of rows: the tree needs it


def test_validate_to_file_default_is_untouched():
    p = inspect.signature(writers.validate_to_file).parameters
    assert list(p)[-1] == "uncert_report" and p["uncert_report"].default is False
    assert list(p)[:5] == ["driver", "batches", "gts", "names", "out_dir"]


REFUSALS = (("B=0", "segments"), ("K=0", "sigma columns"), ("K=17", "sigma columns"), ("L=0", "levels"), ("L=129", "levels"),
            ("off=None", "NULL"), ("z=None", "NULL"), ("off=start1", "not at 0"), ("off=descending", "do not ascend"),
            ("off=toomany", "at most"), ("gt=None", "NULL input"))


def test_entry_point_refuses_and_fails_loudly_without_gpu():
    """Every refusal returns 1 with a `uda_uncert_report_np: ` message before a device is touched and leaves the outputs as they
    were; a call that passes the checks fails in HIP's words where there is no device."""
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from uda_amd import capi\n"
            "lib = capi.load()\n"
            "x = np.ones((2, 4)); c = np.ones(2); z = np.zeros(128); s = np.ones((17, 2, 4))\n"
            "offs = dict(ok=np.array([0, 2], np.int64), start1=np.array([1, 2], np.int64), descending=np.array([0, 2, 1], np.int64),\n"
            "            toomany=np.array([0, (1 << 22) + 1], np.int64))\n"
            "outs = [np.full(4096, 7, np.int64) for _ in range(3)] + [np.full(64, 7.0) for _ in range(2)]\n"
            "def call(B=1, K=1, L=100, off='ok', gt=x, z=z):\n"
            "    off = offs[off] if off is not None else None\n"
            "    B = 2 if off is offs['descending'] else B\n"
            "    p = lambda a: None if a is None else a.ctypes.data\n"
            "    rc = lib.uda_uncert_report_np(0, B, K, L, p(off), p(gt), p(x), p(c), p(c), p(s), p(z), *[o.ctypes.data for o in outs])\n"
            "    same = all((o == 7).all() for o in outs)\n"
            "    print('%%d|%%d|%%s' %% (rc, same, lib.uda_last_error(None).decode()))\n"
            "for kw in %r:\n"
            "    k, v = kw.split('=')\n"
            "    call(**{k: (None if v == 'None' else int(v) if v.isdigit() else v)})\n"
            "call()\n" % (ROOT, [r[0] for r in REFUSALS]))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [line.split("|", 2) for line in out.stdout.splitlines() if "|" in line]
    assert len(rows) == len(REFUSALS) + 1, out.stdout
    for (what, word), (rc, same, msg) in zip(REFUSALS, rows):
        assert rc == "1" and same == "1" and msg.startswith("uda_uncert_report_np: ") and word in msg, (what, msg)
    rc, same, msg = rows[-1]
    assert rc == "1" and msg.startswith("uda_uncert_report_np: ") and not any(w in msg for _, w in REFUSALS), msg
