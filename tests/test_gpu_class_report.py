"""uda_class_report_np on the device against the numpy mirror of its contract (tests/class_report_ref.py): every run goes through the
C ABI (`class_report.report_np`).

Integers are equal.  The float64 sums are the mirror's tree BIT FOR BIT (a NaN where the mirror has one): the device adds the same
terms in the same tree, every operation rounded on its own.  The one exception is nll_sum, whose terms take the device's `log`:
that is not numpy's `log` bit for bit, each may be off by an ulp of log q (together 4 * 2**-53 * |log q| a term), and trees of
slightly different terms also round differently at their nodes, each within the pairwise bound (log2(N) + 2) * 2**-53 * sum|term|.
So nll_sum is held to 2 * (log2(N) + 2) * 2**-53 * sum|term| + 4 * 2**-53 * sum|log q| - the bound of the uncertainty report's
S_nll with one term a row; a term is -log q, so both sums are the same number.

Sizes: 1 and either side of a wave (63, 64, 65), either side of the run of rows a block takes (255 / 256 / 257: the second is the
largest segment whose block writes the outputs itself, the third the smallest that goes through the tree kernel), two runs + 1
(three run roots padded to four) and four runs + 1 (five padded to eight)."""
import numpy as np
import pytest

import class_report_ref as R
import test_class_report_host as H
from common import FULL_MC, make_images, make_params, make_weights
from uda_amd import capi, class_report as cr

pytestmark = pytest.mark.gpu
RUN = capi.CLASSREP_ROWS
SIZES = sorted({1, 63, 64, 65, 255, 256, 257, 513, 1025, RUN - 1, RUN, RUN + 1, 2 * RUN + 1, 4 * RUN + 1})
INTS, SUMS = ("bin_count", "bin_hits", "tab_counts"), ("bin_sum", "brier_sum")


def make(n, M, C, seed, special=True):
    """M tables of n rows of C probabilities (softmax of seeded logits at M temperatures) and labels; with `special`, rows carry an
    exact 0 and 1, a value exactly on a uniform edge, a tie of the row maximum and a probability below 1e-7 for the label."""
    rng = np.random.default_rng([seed, n, M, C])
    logits = rng.normal(0, 2.5, (n, C))
    prob = np.stack([cr.stable_softmax(logits / (0.6 + 0.4 * m)) for m in range(M)])
    label = np.where(rng.uniform(size=n) < 0.7, prob[0].argmax(axis=1), rng.integers(0, C, n)).astype(np.int32)
    if special and C >= 3:
        e = R.uniform_edges()
        prob[0, 0, :3] = [0.0, 1.0, 0.0]
        prob[0, n // 2, :3] = [e[7], 0.2, 0.1]
        prob[0, n - 1, :3] = [0.45, 0.45, 0.1]
        prob[0, n // 3, label[n // 3]] = 1e-9
    return prob, label


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(nan, 0.0, a).view(np.uint64), np.where(nan, 0.0, b).view(np.uint64))


def check(got, want, prob, label):
    off = want["off"]
    for k in INTS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in SUMS:
        assert same_bits(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:5])
    for b in range(len(off) - 1):
        n = int(off[b + 1] - off[b])
        for m in range(len(prob)):
            g, w = got["nll_sum"][b, m], want["nll_sum"][b, m]
            if n == 0:
                assert g == 0.0 and w == 0.0
                continue
            t = R.nll_abs_terms(prob[m, off[b]:off[b + 1]], label[off[b]:off[b + 1]])
            bound = 2 * (np.log2(n) + 2) * 2.0 ** -53 * t + 4 * 2.0 ** -53 * t
            print("nll_sum segment %d table %d: device %r mirror %r bound %g" % (b, m, g, w, bound))
            assert np.isfinite(w) and abs(g - w) <= bound, (b, m, g, w, bound)


def run_both(prob, label, segments=None, edges=None):
    got = cr.report_np(prob, label, segments, edges)
    want = R.report(prob, label, segments, edges)
    assert np.array_equal(got["edges"], want["edges"]) and np.array_equal(got["n_edges"], want["n_edges"])
    check(got, want, prob, label)
    return got


@pytest.mark.parametrize("n", SIZES)
def test_sizes(n):
    got = run_both(*make(n, 2, 3, seed=1))
    assert got["bin_count"].shape == (1, 2, 4, 12) and (got["bin_count"].sum(axis=3) == n).all()
    assert (n < 4 or got["bin_count"][0, 0, 1, 10] >= 1) and got["tab_counts"][0, 0, 0] >= 1 and not got["bin_count"][..., 11].any()


@pytest.mark.parametrize("C", [1, 2, 3, 128])
def test_classes(C):
    got = run_both(*make(RUN + 1, 1, C, seed=2))
    assert got["bin_count"].shape == (1, 1, C + 1, 12) and (got["bin_count"].sum(axis=3) == RUN + 1).all()
    if C == 1:                                               # one class: every probability is 1 and every label the arg-max
        assert got["bin_count"][0, 0, :, 10].tolist() == [RUN + 1] * 2 and got["bin_hits"][0, 0, :, 10].tolist() == [RUN + 1] * 2


@pytest.mark.parametrize("M", [1, 8])
def test_tables(M):
    got = run_both(*make(2 * RUN + 1, M, 3, seed=3), segments=np.array([0, 70, 2 * RUN + 1], np.int64))
    assert got["nll_sum"].shape == (2, M) and (got["nll_sum"] > 0).all()


@pytest.mark.parametrize("n_edges", [2, 11, 64])
def test_shared_edges(n_edges):
    got = run_both(*make(RUN + 40, 2, 3, seed=4), edges=np.linspace(0.0, 1.0 + 1e-8, n_edges))
    assert got["bin_count"].shape == (1, 2, 4, n_edges + 1) and (got["bin_count"].sum(axis=3) == RUN + 40).all()


def test_edges_of_every_target():
    """One edge row per (segment, table, target), of 2, 11, 64 and other counts: the quantile edges of the rows, and rows cut short
    at both ends, which fill id 0 and the id past the last edge."""
    prob, label = make(2 * RUN + 9, 2, 3, seed=5)
    off = np.array([0, 300, 300, 2 * RUN + 9], np.int64)
    rows = cr.quantile_edges(prob, off)
    assert len(rows) == 3 * 2 * 4
    rows[1], rows[2], rows[5], rows[7] = np.array([0.25, 0.5]), np.linspace(0.1, 0.9, 64), np.linspace(0.0, 1.0 + 1e-8, 11), np.linspace(0.3, 0.6, 37)
    got = run_both(prob, label, off, rows)
    assert got["n_edges"][[1, 2, 5, 7]].tolist() == [2, 64, 11, 37] and got["bin_count"].shape == (3, 2, 4, 65)
    assert got["bin_count"][0, 0, 1, 0] > 0 and got["bin_count"][0, 0, 1, 2] > 0 and got["bin_count"][0, 0, 2, 64] > 0
    assert not got["bin_count"][1].any() and (got["bin_count"][[0, 2]].sum(axis=3) == np.array([300, RUN * 2 - 291])[:, None, None]).all()


def test_empty_segments_and_ragged_boundaries():
    prob, label = make(3 * RUN + 40, 2, 3, seed=6)
    off = np.array([0, 0, 100, 100, 100 + RUN + 3, 3 * RUN + 40, 3 * RUN + 40], np.int64)
    got = run_both(prob, label, off)
    for b in (0, 2, 5):
        assert all(not got[k][b].any() for k in INTS + SUMS + ("nll_sum",))
    none = run_both(np.zeros((2, 0, 3)), np.zeros(0, np.int32))
    assert all(not none[k].any() for k in INTS + SUMS + ("nll_sum",))


def test_all_rows_identical():
    n = 2 * RUN + 1
    prob = np.tile(np.array([0.2, 0.7, 0.1]), (2, n, 1))
    got = run_both(prob, np.ones(n, np.int32))
    assert set(np.unique(got["bin_count"])) <= {0, n} and got["bin_hits"][0, 0, :, :].sum(axis=1).tolist() == [0, n, 0, n]


def test_row_permutation_leaves_the_integers():
    prob, label = make(2 * RUN + 1, 2, 3, seed=7)
    off = np.array([0, 70, 2 * RUN + 1], np.int64)
    a = cr.report_np(prob, label, off)
    rng = np.random.default_rng(8)
    perm = np.concatenate([rng.permutation(70), 70 + rng.permutation(2 * RUN + 1 - 70)])
    b = cr.report_np(prob[:, perm], label[perm], off)
    for k in INTS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_segments_add_up():
    """The rows as one segment, and cut into three: the integer tallies of the three add up to the one's; the first of the three
    equals the same rows alone, sums included."""
    prob, label = make(2 * RUN + 60, 2, 3, seed=9)
    n = RUN + 1
    one = cr.report_np(prob, label)
    three = cr.report_np(prob, label, np.array([0, n, n + 7, len(label)], np.int64))
    alone = cr.report_np(prob[:, :n], label[:n])
    for k in INTS:
        np.testing.assert_array_equal(three[k].sum(axis=0), one[k][0], err_msg=k)
        np.testing.assert_array_equal(alone[k][0], three[k][0], err_msg=k)
    assert all(same_bits(alone[k][0], three[k][0]) for k in SUMS + ("nll_sum",))


def test_nan_and_infinite_probabilities():
    prob, label = make(RUN + 5, 2, 3, seed=10)
    prob[0, 5] = [0.3, np.nan, 0.9]                          # the arg-max is the NaN, not the 0.9
    prob[0, 6] = [np.nan, np.nan, 0.2]                       # ... the first of them
    prob[0, 70] = [np.inf, 0.1, 0.2]
    prob[0, 71] = [0.5, -np.inf, 0.2]
    prob[0, 200] = [0.0, 0.0, 0.0]                           # a row sum of 0
    prob[1, RUN + 1] = [1.5, -0.25, 0.1]                     # finite, outside [0, 1]
    label[[5, 6, 70, 71]] = [1, 0, 0, 2]
    got = run_both(prob, label)
    rep = cr.ClassReport(got)
    assert got["tab_counts"][0, 0, 1] == 5 and got["tab_counts"][0, 1, 1] == 0
    assert rep.overflow_count(0, 0) == 2 and rep.overflow_count(0, 1) == 2 and rep.overflow_count(0, 2) == 0       # NaN, inf | NaN, NaN
    assert rep.overflow_count(0, "all") == 3 and got["bin_hits"][0, 0, 3, 11] == 3                                 # rows 5, 6, 70: all hits
    assert np.isnan(got["bin_sum"][0, 0, 3, 11]) and got["bin_count"][0, 0, 1, 0] == 1 and got["bin_sum"][0, 0, 1, 0] == -np.inf
    assert rep.overflow_count(1, 0) == 1 and got["bin_count"][0, 1, 1, 0] == 1 and got["bin_sum"][0, 1, 1, 0] == -0.25
    with pytest.raises(IndexError):
        rep.bins(0, "all")
    assert rep.bins(0, "all", overflow="last")["bin_count"].sum() == RUN + 5


def test_refusals_leave_the_outputs_untouched():
    env = {}
    exec(H.REFUSAL_SETUP, env)
    for kw, word in H.REFUSALS:
        rc, same, msg = env["call"](**env["kwargs"](kw))
        assert rc == 1 and same and msg.startswith("uda_class_report_np: ") and word in msg, (kw, msg)
    rc, same, msg = env["call"]()
    outs = env["outs"]
    assert rc == 0 and not same and outs[0][:48].sum() == 2 * 4 and outs[0][3] == 2 and outs[5][:2].tolist() == [0, 0]


def test_driver_path_returns_the_report_of_the_matched_rows(tmp_path):
    """A tiny synthetic model through validate_to_file(..., class_report=models): the report it returns is the one `from_filtered`
    gives for the returned matched rows through the mirror - integers equal, sums the same bits; without the switch nothing is
    added."""
    from uda_amd import writers
    from uda_amd.calibration import IsoTable
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
            ranks = rng.integers(0, max(int(det[3][i]), 1), 5)
            gb[i, :5] = det[0][i, ranks, :4] + rng.normal(0, 0.5, (5, 4)).astype(np.float32)
            gc[i, :5] = rng.integers(1, d.num_classes + 1, 5)
        plain = writers.validate_to_file(d, [batch], [(gb, gc)], [["a.png", "b.png"]], str(tmp_path / "plain"))
        assert "class_report" not in plain
        C = d.num_classes
        xs = np.array([0.0, 0.2, 0.5, 1.0])
        models = {"ts_all": np.float32(1.4), "ts_percls": np.linspace(0.8, 1.9, C).astype(np.float32),
                  "iso_all": IsoTable(xs, xs ** 1.5), "iso_percls": [IsoTable(xs, xs ** (1 + 0.1 * c)) for c in range(C)]}
        f = writers.validate_to_file(d, [batch], [(gb, gc)], [["a.png", "b.png"]], str(tmp_path / "report"), class_report=models)
        rep = f["class_report"]
        assert rep.names == ["", "all_calib_TS", "perclass_calib_TS", "all_calib_IR", "perclass_calib_IR"]
        assert rep.n_rows.tolist() == [len(f["names"])] == [10] and rep.C == C
        want = cr.from_filtered(f, models, split=0, one_based=True, engine=R.report)
        for k in INTS:
            np.testing.assert_array_equal(getattr(rep, k), getattr(want, k), err_msg=k)
        assert all(same_bits(getattr(rep, k), getattr(want, k)) for k in SUMS)
        assert len(cr.title_lines(rep, "all_calib_IR", "all")) == 2 and cr.title_lines(rep, "", 0) == cr.title_lines(want, "", 0)
        for k in plain:
            if isinstance(plain[k], np.ndarray):
                assert np.array_equal(plain[k], f[k], equal_nan=True), k
    finally:
        d.close()
