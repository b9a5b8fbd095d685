"""The classification calibration report on the host (`class_report`; reference src/calibrate_classification.py:97-143, 250-440)
without a GPU: the numpy mirror of the contract (tests/class_report_ref.py) against what the reference's own `_calibr_bins` and
`stable_softmax` gave (tests/golden/class_report_golden.npz, maker beside it), then `ClassReport`, `title_lines`,
`tables_from_logits`, `merge`, the overflow rule and `from_filtered` on mirror output (`engine=`).

Counts, hits (so `freq`), the selection of the non-empty bins, `bin_prob` and `bin_count` are equal.  A bin's sum of probabilities
is `np.bincount`'s running sum in the reference and the root of the zero-padded pairwise tree here: two summations of the same
terms.  With u = 2**-53, a running sum of n terms is within gamma(n - 1) * sum|term| of the exact sum and the tree, whose depth is
ceil(log2 n), within gamma(ceil(log2 n) + 1) * sum|term| (gamma(k) = k u / (1 - k u), Higham); n is taken as the segment's row
count, no smaller than any bin's.  So the sums differ by at most

    SUM_BOUND(n, terms) = (gamma(n - 1) + gamma(ceil(log2 n) + 1)) * sum|term|

and what is formed from them follows by propagation, every division, subtraction and product adding one rounding (u, relative) on
either side:  prob = sum / count: SUM_BOUND / count + 2 u |prob|;  MCE = max|freq - prob|: the largest prob bound + 2 u MCE;
ECE = sum |freq - prob| * (count / n) over k <= 10 bins: sum (count / n) * (prob bound) + 2 (k + 1) u ECE (the subtraction, the
product and the k - 1 additions on either side);  Brier = mean of (p - y)**2, whose terms are the same bits on both sides, numpy's
mean being some order of additions: SUM_BOUND / n + 2 u Brier, over n C terms (and C - 1 more additions here) for `brier_all`.
The bounds are printed."""
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import class_report_ref as R
from common import ROOT
from uda_amd import capi, class_report as cr, writers
from uda_amd.calibration import IsoTable

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "class_report_golden.npz"))
CASES = ("n1", "n7", "n300")
STRATEGIES = ("uniform", "quantile")
TARGETS = (0, 1, 2, "all")
U = 2.0 ** -53


def gamma(k):
    return k * U / (1 - k * U)


def sum_bound(n, abs_sum, extra=0):
    return (gamma(max(n - 1, 0)) + gamma(math.ceil(math.log2(max(n, 1))) + 1 + extra)) * abs_sum


def inputs(case):
    return GOLD[case + "_prob"], GOLD[case + "_label"]


def edges_for(case, strategy):
    p, _ = inputs(case)
    return None if strategy == "uniform" else cr.quantile_edges(p[None])


def gold(case, strategy, t, key):
    return GOLD["%s_%s_t%s_%s" % (case, strategy, t, key)]


def target_values(p, t):
    return p[:, t] if t != "all" else p[np.arange(len(p)), p.argmax(axis=1)]


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("case", CASES)
def test_mirror_reproduces_the_reference(case, strategy):
    p, label = inputs(case)
    n = len(p)
    rep = cr.report(p[None], label, edges=edges_for(case, strategy), engine=R.report)
    assert rep.names == ["0"] and len(rep) == 1 and rep.C == 3
    for t in TARGETS:
        g = lambda k: gold(case, strategy, t, k)                                # noqa: E731
        b = rep.bins(0, t)
        assert rep.overflow_count(0, t) == 0                                      # (the reference did not raise either)
        assert np.array_equal(b["bin_count"], g("bin_count")) and np.array_equal(b["bin_prob"], g("bin_prob"))
        assert np.array_equal(b["freq"], g("freq")) and b["prob"].shape == g("prob").shape
        x = target_values(p, t)
        ids = R.bin_ids(x, rep.target_edges(0, t))
        filled = [k for k in range(len(rep.target_edges(0, t))) if (ids == k).any()]
        prob_bound = np.array([sum_bound(n, np.abs(x[ids == k]).sum()) / c + 2 * U * abs(pr)
                               for k, c, pr in zip(filled, b["bin_count"], g("prob"))])
        assert (np.abs(b["prob"] - g("prob")) <= prob_bound).all(), (case, strategy, t, b["prob"] - g("prob"), prob_bound)
        ece_bound = np.sum(b["bin_count"] / n * prob_bound) + 2 * (len(filled) + 1) * U * max(rep.ece(0, t), float(g("ece")))
        mce_bound = prob_bound.max() + 2 * U * max(rep.mce(0, t), float(g("mce")))
        print("%s %s target %s: prob bound %.3g, ECE %r (reference %r, bound %.3g), MCE %r (reference %r, bound %.3g)" %
              (case, strategy, t, prob_bound.max(), rep.ece(0, t), float(g("ece")), ece_bound, rep.mce(0, t), float(g("mce")), mce_bound))
        assert abs(rep.ece(0, t) - g("ece")) <= ece_bound and abs(rep.mce(0, t) - g("mce")) <= mce_bound
    y = np.eye(3)[label]
    for t in range(3):
        bound = sum_bound(n, ((p[:, t] - y[:, t]) ** 2).sum()) / n + 2 * U * GOLD[case + "_brier"][t]
        print("%s Brier class %d: %r (reference %r, bound %.3g)" % (case, t, rep.brier(0, t), GOLD[case + "_brier"][t], bound))
        assert abs(rep.brier(0, t) - GOLD[case + "_brier"][t]) <= bound
    bound = sum_bound(3 * n, ((p - y) ** 2).sum(), extra=2) / (3 * n) + 2 * U * float(GOLD[case + "_brier_all"])
    assert abs(rep.brier_all(0) - GOLD[case + "_brier_all"]) <= bound, (rep.brier_all(0), GOLD[case + "_brier_all"], bound)


@pytest.mark.parametrize("case", CASES)
def test_quantile_edges_are_the_reference_s(case):
    p, _ = inputs(case)
    rows = cr.quantile_edges(p[None])
    assert len(rows) == 4
    for t, row in zip(TARGETS, rows):
        want = gold(case, "quantile", t, "edges")
        if len(want) == 1:                                   # all values equal (n1): -inf in front, see quantile_edges
            assert row[0] == -np.inf and np.array_equal(row[1:], want)
        else:
            assert np.array_equal(row, want)
        assert np.array_equal(cr.quantile_edges(target_values(p, t)), row)
    assert np.array_equal(cr.uniform_edges(), GOLD["uniform_edges"]) and np.array_equal(R.uniform_edges(), GOLD["uniform_edges"])
    assert np.array_equal(gold(case, "uniform", 0, "edges"), GOLD["uniform_edges"])


def test_planted_rows():
    p, label = inputs("n7")
    e = GOLD["uniform_edges"]
    rep = cr.report(p[None], label, engine=R.report)
    assert p[1, 0] == e[3] and R.bin_ids(p[1, :1], e)[0] == 4 == np.digitize(e[3], e)     # on an edge: the bin above it, id 4
    assert rep.bin_count[0, 0, 0, 4] == 3                             # (with 0.33 and 0.4)
    assert rep.bin_count[0, 0, 0, 1] == 2 and rep.bin_count[0, 0, 1, 10] == 1    # p = 0 -> id 1 (with 0.05), p = 1 -> id 10
    assert R.argmax_rule(p)[2] == 0 and p[2, 0] == p[2, 1]           # the tie: the first maximum
    assert rep.bin_hits[0, 0, 3].sum() == np.count_nonzero(label == p.argmax(axis=1))
    big = cr.report(GOLD["n300_prob"][None], GOLD["n300_label"], engine=R.report)
    assert big.bin_count[0, 0, 1, 6] == 0 and big.bin_count[0, 0, 1, 5] > 0 and big.bin_count[0, 0, 1, 7] > 0   # an empty bin in the middle
    assert (big.bin_count[0, 0].sum(axis=1) == 300).all() and not big.bin_count[0, 0, :, 0].any() and not big.bin_count[0, 0, :, 11].any()


def test_stable_softmax_is_the_reference_s():
    for k in ("n300", "c10"):
        got = cr.stable_softmax(GOLD[k + "_logits"])
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), GOLD[k + "_softmax"].view(np.uint32))


def test_nll_is_the_stated_formula():
    p, label = inputs("n300")
    rep = cr.report(p[None], label, engine=R.report)
    q = p[np.arange(300), label] / ((p[:, 0] + p[:, 1]) + p[:, 2])
    terms = -np.log(np.clip(q, 1e-7, 1 - 1e-7))
    assert rep.count("left_out") == 0 and rep.count("clipped") == np.count_nonzero((q < 1e-7) | (q > 1 - 1e-7)) >= 1
    bound = sum_bound(300, np.abs(terms).sum()) / 300 + 2 * U * terms.mean()
    assert abs(rep.nll() - terms.mean()) <= bound
    # a row with a non-finite entry, and a row that sums to 0, are left out and counted
    p2 = np.array([[0.2, 0.8, 0.0], [np.nan, 0.5, 0.5], [0.0, 0.0, 0.0], [0.5, -0.5, 0.0], [np.inf, 0.1, 0.1], [1.0, 0.0, 0.0]])
    rep = cr.report(p2[None], [1, 1, 0, 0, 0, 1], engine=R.report, overflow="last")
    assert rep.count("left_out") == 4 and rep.count("clipped") == 1
    assert rep.nll() == (-np.log(0.8 / (0.2 + 0.8 + 0.0)) + -np.log(1e-7)) / 2


def iso_tables():
    xs = np.array([0.0, 0.1, 0.35, 0.6, 1.0])
    return [IsoTable(xs, np.array([0.0, 0.02, 0.3, 0.7, 1.0]) ** (1 + 0.3 * i)) for i in range(3)]


def softmax_rows(logits):                                    # the reference's loop, row by row
    return np.asarray([np.exp(x - max(x)) / np.sum(np.exp(x - max(x))) for x in logits])


def test_tables_from_logits():
    logits = GOLD["n300_logits"]
    isos = iso_tables()
    temps = np.array([1.5, 0.8, 2.0], np.float32)
    tabs, names = cr.tables_from_logits(logits, ts_all=np.float32(1.7), ts_percls=temps, iso_all=isos[0], iso_percls=isos)
    assert names == ["", "all_calib_TS", "perclass_calib_TS", "all_calib_IR", "perclass_calib_IR"]
    assert tabs.shape == (5, 300, 3) and tabs.dtype == np.float64
    soft = GOLD["n300_softmax"]
    assert np.array_equal(tabs[0], soft.astype(np.float64))
    assert np.array_equal(tabs[1], softmax_rows(logits / np.float32(1.7)).astype(np.float64))
    assert np.array_equal(tabs[2], softmax_rows(logits / temps).astype(np.float64))
    one = np.interp(np.clip(soft.flatten().astype(np.float64), 0, 1), isos[0].x, isos[0].y).astype(np.float32).reshape(soft.shape)
    assert np.array_equal(tabs[3], (one / np.stack([np.sum(one, axis=-1)] * 3, axis=-1)).astype(np.float64))
    per = np.stack([np.interp(soft[:, i].astype(np.float64), isos[i].x, isos[i].y).astype(np.float32) for i in range(3)], axis=1)
    assert np.array_equal(tabs[4], (per / np.stack([np.sum(per, axis=-1)] * 3, axis=-1)).astype(np.float64))
    assert cr.tables_from_logits(logits)[1] == [""] and cr.tables_from_logits(logits, iso_all=isos[1])[1] == ["", "all_calib_IR"]
    with pytest.raises(ValueError, match="3 temperatures"):
        cr.tables_from_logits(logits, ts_percls=[1.0, 2.0])
    with pytest.raises(ValueError, match="3 IsoTables"):
        cr.tables_from_logits(logits, iso_percls=isos[:2])


def reference_title(case, t, nll=None, sce=None):
    ece, mce = float(gold(case, "uniform", t, "ece")), float(gold(case, "uniform", t, "mce"))
    if t != "all":
        return ("ECE " + str(np.around(ece, 3)) + "\nMCE " + str(np.around(mce, 3)) + "     Brier: " +
                str(np.around(GOLD[case + "_brier"][t], 3))).split("\n")
    return ("ECE " + str(np.around(ece, 3)) + "     NLL: " + str(np.around(nll, 3)) + "     SCE: " + str(np.around(sce, 3)) + "\n" + "MCE " +
            str(np.around(mce, 3)) + "     Brier: " + str(np.around(float(GOLD[case + "_brier_all"]), 3))).split("\n")


@pytest.mark.parametrize("case", CASES)
def test_title_lines(case):
    """The titles from the mirror's report are those formed from the reference's own numbers, character for character (no number
    of the committed cases lies within its bound of a rounding boundary of the third decimal)."""
    p, label = inputs(case)
    rep = cr.report({"": p}, label, engine=R.report)
    assert rep.names == [""]
    for t in range(3):
        assert cr.title_lines(rep, "", t) == reference_title(case, t)
    sce = np.mean([np.around(float(gold(case, "uniform", t, "ece")), 3) for t in range(3)])
    assert rep.sce("") == sce
    lines = cr.title_lines(rep, "", "all")
    assert lines == reference_title(case, "all", rep.nll(""), sce) and len(lines) == 2
    assert lines[0].startswith("ECE ") and "     NLL: " in lines[0] and "     SCE: " in lines[0] and lines[1].startswith("MCE ")
    assert cr.title_lines(rep, "", "all", quantile=True)[0].startswith("ACE ")


def test_merge():
    p, label = inputs("n300")
    tabs, names = cr.tables_from_logits(GOLD["n300_logits"], ts_all=np.float32(1.7))
    tabs[0] = p
    whole = cr.report(tabs, label, names, engine=R.report)
    for cut, exact in ((256, True), (150, False)):
        a, b = (cr.report(tabs[:, rows], label[rows], names, engine=R.report) for rows in (slice(0, cut), slice(cut, 300)))
        m = a.merge(b)
        for k in cr.ClassReport.INT_KEYS + ("n_rows", "off"):
            assert np.array_equal(getattr(m, k), getattr(whole, k)), k
        for t in TARGETS:
            bm, bw = m.bins(1, t), whole.bins(1, t)
            assert all(np.array_equal(bm[k], bw[k]) for k in ("freq", "bin_prob", "bin_count"))
        if exact:                                            # 256 rows, then 44: the whole's tree has exactly these two subtrees
            assert all(np.array_equal(getattr(m, k), getattr(whole, k)) for k in cr.ClassReport.SUM_KEYS)
        else:
            assert np.allclose(m.bin_sum, whole.bin_sum, rtol=0, atol=sum_bound(300, 300.0))
    with pytest.raises(ValueError, match="same tables"):
        whole.merge(cr.report(tabs[:1], label, [""], engine=R.report))
    with pytest.raises(ValueError, match="same tables"):
        whole.merge(cr.report(tabs, label, names, edges=np.linspace(0, 1 + 1e-8, 6), engine=R.report))


def test_overflow_rule():
    p = np.array([[0.2, 0.3, 0.5], [0.1, 1.5, 0.4], [np.nan, 0.2, 0.8], [0.95, 0.03, 0.02]])
    label = [2, 1, 0, 0]
    rep = cr.report(p[None], label, engine=R.report)
    assert rep.overflow_count(0, 0) == 1 and rep.overflow_count(0, 1) == 1 and rep.overflow_count(0, 2) == 0 and rep.overflow_count(0, "all") == 2
    assert rep.bins(0, 2)["bin_count"].sum() == 4            # class 2 is clean
    for t in (0, 1, "all"):
        with pytest.raises(IndexError, match="boolean index did not match"):
            rep.bins(0, t)
        with pytest.raises(IndexError):
            rep.ece(0, t)
    with pytest.raises(IndexError):
        cr.title_lines(rep)
    b = rep.bins(0, 1, overflow="last")
    assert b["bin_count"].tolist() == [1, 1, 1, 1] and b["bin_prob"].tolist()[-1] == 1 + 1e-8 and b["freq"][-1] == 1.0 and b["prob"][-1] == 1.5
    folded = cr.report(p[None], label, engine=R.report, overflow="last")
    assert folded.bins(0, "all")["bin_count"].sum() == 4 and np.isnan(folded.bins(0, "all")["prob"][-1])
    # the arg-max rule: the first NaN of row 2, else the first maximum
    assert R.argmax_rule(p).tolist() == [2, 1, 0, 0] == cr.argmax_rows(p).tolist()
    with pytest.raises(ValueError, match="overflow"):
        cr.report(p[None], label, engine=R.report, overflow="drop")


def test_from_filtered_takes_the_evaluation_split():
    rng = np.random.default_rng(4)
    logits = rng.normal(0, 2, (53, 3)).astype(np.float32)
    filtered = {"logits": logits, "gt_classes": rng.integers(0, 3, 53).astype(np.float32)}
    models = {"ts_all": np.float32(1.3), "iso_percls": iso_tables()}
    rep = cr.from_filtered(filtered, models, engine=R.report)
    assert rep.names == ["", "all_calib_TS", "perclass_calib_IR"] and rep.n_rows.tolist() == [53 - int(53 * 0.8)]
    tabs, names = cr.tables_from_logits(logits[42:], ts_all=np.float32(1.3), iso_percls=iso_tables())
    want = cr.report(tabs, filtered["gt_classes"][42:], names, engine=R.report)
    assert all(np.array_equal(getattr(rep, k), getattr(want, k)) for k in cr.ClassReport.INT_KEYS + cr.ClassReport.SUM_KEYS)
    assert cr.from_filtered(filtered, None, split=0, engine=R.report).n_rows.tolist() == [53]
    one = dict(filtered, gt_classes=filtered["gt_classes"] + 1)
    assert np.array_equal(cr.from_filtered(one, models, one_based=True, engine=R.report).bin_hits, rep.bin_hits)
    q = cr.from_filtered(filtered, models, quantile=True, engine=R.report)
    assert len(q.n_edges) == 3 * 4 and q.bins("all_calib_TS", 1)["bin_count"].sum() == 11
    with pytest.raises(ValueError, match="no logits"):
        cr.from_filtered({"logits": None, "gt_classes": []}, engine=R.report)
    with pytest.raises(ValueError, match="no such calibration models"):
        cr.from_filtered(filtered, {"ts_percoo": 1.0}, engine=R.report)


def test_inputs_are_checked_before_the_library():
    p, label = inputs("n7")
    with pytest.raises(ValueError, match="7 rows, 6 labels"):
        cr.report_np(p[None], label[:6])
    with pytest.raises(ValueError, match="outside 0..2"):
        cr.report_np(p[None], np.full(7, 3))
    with pytest.raises(ValueError, match="1..8"):
        cr.report_np(np.stack([p] * 9), label)
    with pytest.raises(ValueError, match="segments must ascend"):
        cr.report_np(p[None], label, segments=[0, 5, 4, 7])
    with pytest.raises(ValueError, match="do not ascend strictly"):
        cr.report_np(p[None], label, edges=[0.0, 0.5, 0.5, 1.0])
    with pytest.raises(ValueError, match="edge rows"):
        cr.report_np(p[None], label, edges=[[0.0, 1.0]] * 3)
    with pytest.raises(ValueError, match="2..64"):
        cr.report_np(p[None], label, edges=np.linspace(0, 1, 65))


def test_binding_and_limits_match_the_header():
    text = open(capi.HEADER).read()
    for name, value in (("UDA_CLASSREP_ROWS", capi.CLASSREP_ROWS), ("UDA_CLASSREP_MAX_B", capi.CLASSREP_MAX_B),
                        ("UDA_CLASSREP_MAX_M", capi.CLASSREP_MAX_M), ("UDA_CLASSREP_MAX_C", capi.CLASSREP_MAX_C),
                        ("UDA_CLASSREP_MAX_E", capi.CLASSREP_MAX_E), ("UDA_CLASSREP_MAX_ROWS", capi.CLASSREP_MAX_ROWS)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value
    assert (capi.CLASSREP_MAX_B, capi.CLASSREP_MAX_M, capi.CLASSREP_MAX_C, capi.CLASSREP_MAX_E, capi.CLASSREP_MAX_ROWS) == (4096, 8, 128, 64, 1 << 22)
    assert re.search(r"\bint uda_class_report_np\(int32_t device,", text)
    assert "uda_class_report_np   <-" in text and "calibrate_classification.py:97-143, 250-440" in text.split("Conventions:")[0]
    assert "uda_class_report_np" in capi.EXPORTS and len(capi._SIGNATURES["uda_class_report_np"][1]) == 17
    assert capi.CLASSREP_ROWS & (capi.CLASSREP_ROWS - 1) == 0    # a run is a power of two of rows: the tree needs it


def test_validate_to_file_default_is_untouched():
    p = inspect.signature(writers.validate_to_file).parameters
    assert p["class_report"].default is None and list(p)[-1] == "uncert_report" and p["uncert_report"].default is False
    assert list(p)[:9] == ["driver", "batches", "gts", "names", "out_dir", "box_calibrator", "class_calibrator", "occlusions", "truncations"]


REFUSALS = (("B=0", "segments"), ("B=4097", "segments"), ("M=0", "probability tables"), ("M=9", "probability tables"), ("C=0", "classes"),
            ("C=129", "classes"), ("E=1", "edges a row"), ("E=65", "edges a row"), ("G=2", "edge rows"), ("off=None", "NULL"),
            ("edges=None", "NULL"), ("ne=None", "NULL"), ("off=start1", "not at 0"), ("off=descending", "do not ascend"),
            ("off=toomany", "at most"), ("prob=None", "NULL input"), ("label=None", "NULL input"), ("label=high", "outside 0..2"),
            ("label=negative", "outside 0..2"), ("edges=tie", "do not ascend strictly"), ("edges=nan", "do not ascend strictly"),
            ("ne=one", "holds 1 edges"), ("ne=many", "holds 12 edges"))
REFUSAL_SETUP = ("import numpy as np\n"
                 "from uda_amd import capi\n"
                 "lib = capi.load()\n"
                 "prob = np.full((1, 2, 3), 0.25); e = np.linspace(0, 1 + 1e-8, 11)\n"
                 "tie = e.copy(); tie[4] = tie[3]; nan = e.copy(); nan[10] = np.nan\n"
                 "vals = dict(ok=np.array([0, 2], np.int64), start1=np.array([1, 2], np.int64), descending=np.array([0, 2, 1], np.int64),\n"
                 "            toomany=np.array([0, (1 << 22) + 1], np.int64), high=np.array([0, 3], np.int32), negative=np.array([-1, 0], np.int32),\n"
                 "            tie=tie, nan=nan, one=np.array([1], np.int32), many=np.array([12], np.int32))\n"
                 "outs = [np.full(64, 7, np.int64) for _ in range(2)] + [np.full(64, 7.0) for _ in range(3)] + [np.full(64, 7, np.int64)]\n"
                 "def call(B=1, M=1, C=3, G=1, E=11, off='ok', prob=prob, label=np.array([0, 2], np.int32), edges=e, ne=np.array([11], np.int32)):\n"
                 "    off, prob, label, edges, ne = (vals[a] if isinstance(a, str) else a for a in (off, prob, label, edges, ne))\n"
                 "    B = 2 if off is vals['descending'] else B\n"
                 "    p = lambda a: None if a is None else a.ctypes.data\n"
                 "    rc = lib.uda_class_report_np(0, B, M, C, G, E, p(off), p(prob), p(label), p(edges), p(ne), *[o.ctypes.data for o in outs])\n"
                 "    same = all((o == 7).all() for o in outs)\n"
                 "    return rc, same, lib.uda_last_error(None).decode()\n"
                 "def kwargs(kw):\n"
                 "    k, v = kw.split('=')\n"
                 "    return {k: (None if v == 'None' else int(v) if v.isdigit() else v)}\n")


def test_entry_point_refuses_and_fails_loudly_without_gpu():
    """Every refusal returns 1 with a `uda_class_report_np: ` message before a device is touched and leaves the outputs as they
    were; a call that passes the checks fails in HIP's words where there is no device."""
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    code = ("import sys; sys.path.insert(0, %r)\n" % ROOT + REFUSAL_SETUP +
            "for kw in %r + ['']:\n"
            "    print('%%d|%%d|%%s' %% call(**(kwargs(kw) if kw else {})))\n" % ([r[0] for r in REFUSALS],))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [line.split("|", 2) for line in out.stdout.splitlines() if "|" in line]
    assert len(rows) == len(REFUSALS) + 1, out.stdout
    for (what, word), (rc, same, msg) in zip(REFUSALS, rows):
        assert rc == "1" and same == "1" and msg.startswith("uda_class_report_np: ") and word in msg, (what, msg)
    rc, same, msg = rows[-1]
    assert rc == "1" and msg.startswith("uda_class_report_np: ") and not any(w in msg for _, w in REFUSALS), msg
