"""Set similarity on the device (`set_similarity.nn_dist2` / `emp_kl_divergences` / `jensen_shannon_divergences` /
`calculate_set_similarity` -> `uda_nn_dist2_np`; reference active_learning_eval.py:458-583, 946-1029): the C entry point and the
package against the numpy mirror (tests/knn_ref.py) bit for bit at every size where the tiling changes (queries per block,
reference points per staged chunk, from include/uda_hip.h), with nearest neighbours planted across those boundaries and across
span ends, ragged batches, the refusals, and the reference's own values (tests/golden/similarity_golden.npz).  A minimum of
individually rounded sums does not depend on the order it is taken in: there is no tolerance anywhere."""
import os
import re

import numpy as np
import pytest

import knn_ref as R
from common import ROOT
from uda_amd import capi
from uda_amd import set_similarity as S

pytestmark = pytest.mark.gpu

_DEFS = dict(re.findall(r"#define (UDA_KNN_[A-Z_]+) (\d+)", open(os.path.join(ROOT, "include", "uda_hip.h")).read()))
ROWS, COLS, MAX_N = int(_DEFS["UDA_KNN_ROWS"]), int(_DEFS["UDA_KNN_COLS"]), int(_DEFS["UDA_KNN_MAX_N"])
SIZES = [1, 2, 63, 64, 65, ROWS - 1, ROWS, ROWS + 1, COLS - 1, COLS, COLS + 1, 2 * COLS + 3]
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "similarity_golden.npz"))
KL_CASES = [str(c) for c in GOLD["kl_cases"]]
JSD_CASES = [str(c) for c in GOLD["jsd_cases"]]
SENTINEL = -7.0
TINY = 2.0 ** -30          # planted neighbours lie this far away in one coordinate; random points of the unit cube do not


def call(D, q_off, r_off, queries, refs, self, out, B=None, device=0):
    lib = capi.load()
    q_off, r_off = np.asarray(q_off, np.int64), np.asarray(r_off, np.int64)
    rc = lib.uda_nn_dist2_np(device, D, len(q_off) - 1 if B is None else B, queries.ctypes.data, q_off.ctypes.data, refs.ctypes.data,
                             r_off.ctypes.data, None if self is None else self.ctypes.data, out.ctypes.data)
    return rc, lib.uda_last_error(None).decode()


def raw(problems, self_null=False):
    """One call of the C entry point on [(queries, refs, self flag)]: the d2 arrays.  The output buffer is one element longer than
    asked for and must keep its sentinel there."""
    D = problems[0][0].shape[1]
    q_off = np.concatenate([[0], np.cumsum([q.shape[0] for q, _, _ in problems])])
    r_off = np.concatenate([[0], np.cumsum([r.shape[0] for _, r, _ in problems])])
    queries = np.ascontiguousarray(np.concatenate([q for q, _, _ in problems]), np.float64)
    refs = np.ascontiguousarray(np.concatenate([r for _, r, _ in problems]), np.float64)
    self = None if self_null else np.array([s for _, _, s in problems], np.uint8)
    out = np.full(int(q_off[-1]) + 1, SENTINEL)
    rc, msg = call(D, q_off, r_off, queries, refs, self, out)
    assert rc == 0, msg
    assert out[-1] == SENTINEL
    return [out[a:b] for a, b in zip(q_off[:-1], q_off[1:])]


def cube(n, D, *seed):
    return np.random.default_rng([n, D, *seed]).random((n, D))


def beside(point, k=0):
    out = point.copy()
    out[k % out.size] += TINY
    return out


@pytest.mark.parametrize("D", [1, 3, 4])
@pytest.mark.parametrize("n", SIZES)
def test_entry_point_equals_the_mirror(n, D):
    """n queries against every m of the sweep, and the set of n against itself; a second call gives the same bits."""
    q = cube(n, D, 0)
    for m in SIZES:
        r = cube(m, D, 1)
        want = R.dist2(q, r)
        got, = raw([(q, r, 0)])
        assert np.array_equal(got, want), (n, m, D)
        again, = raw([(q, r, 0)])
        assert np.array_equal(again, got)
    want = R.dist2(q, q, self=True)
    got, = raw([(q, q, 1)])
    assert np.array_equal(got, want) and (n == 1 or (got > 0).all())
    assert np.array_equal(raw([(q, q, 1)])[0], got)
    assert np.array_equal(S.nn_dist2([(q, None)])[0], want) and np.array_equal(S.nn_dist2([(q, cube(65, D, 1))])[0], R.dist2(q, cube(65, D, 1)))


@pytest.mark.parametrize("D", [1, 3, 4])
def test_planted_neighbours_at_the_boundaries(D):
    """Each planted reference is the unique nearest of its query: its d2 is TINY^2 exactly and is found whichever thread, block and
    chunk it falls into."""
    n, m = 2 * ROWS, 2 * COLS + 3
    q, r = cube(n, D, 2), cube(m, D, 3)
    planted = [(ROWS - 1, COLS), (ROWS, COLS - 1), (63, 64), (0, m - 1)]
    for k, (i, j) in enumerate(planted):
        r[j] = beside(q[i], k)
    want = R.dist2(q, r)
    got, = raw([(q, r, 0)])
    assert np.array_equal(got, want)
    for i, j in planted:
        others = R.dist2(q[i:i + 1], np.delete(r, j, axis=0))[0]
        assert got[i] == ((q[i] - r[j]) ** 2).sum() and 0 < got[i] <= 1.01 * TINY * TINY and others > got[i], (i, j, got[i], others)


@pytest.mark.parametrize("D", [1, 3, 4])
def test_self_problem_skips_the_own_row_and_nothing_else(D):
    """Row COLS is an exact copy of row COLS - 1: both are 0, they do not skip each other; every other point's coordinates appear
    nowhere else and its d2 is not 0."""
    n = 2 * COLS + 3
    p = cube(n, D, 4)
    p[COLS] = p[COLS - 1]
    got, = raw([(p, p, 1)])
    assert np.array_equal(got, R.dist2(p, p, self=True))
    assert got[COLS] == 0 and got[COLS - 1] == 0 and (np.delete(got, [COLS - 1, COLS]) > 0).all()
    as_cross, = raw([(p, p, 0)])
    assert (as_cross == 0).all()


def test_spans_of_several_chunks_equal_the_mirror():
    """A self problem of 12 301 points, D = 3: 49 row blocks and 25 reference chunks, more blocks than one wave of them, cut into
    spans of two chunks.  Nearest neighbours planted across span ends, seen from both sides."""
    N = 12301
    p = cube(N, 3, 5)
    planted = [(ROWS - 1, 2 * COLS), (2 * COLS - 1, 24 * COLS), (N - 3, 4 * COLS - 1), (5, N - 1), (6 * COLS, 6 * COLS - 1)]
    for k, (a, b) in enumerate(planted):
        p[b] = beside(p[a], k)
    want = R.dist2(p, p, self=True)
    got, = raw([(p, p, 1)])
    assert np.array_equal(got, want)
    for a, b in planted:
        assert got[a] == ((p[a] - p[b]) ** 2).sum() == got[b] and 0 < got[a] <= 1.01 * TINY * TINY
    assert (got > 0).all() and np.array_equal(S.nn_dist2([(p, None)])[0], want)


def test_ragged_batch_equals_single_problems_and_the_mirror():
    D = 3
    a, b, c, d, e = cube(1, D, 6), cube(ROWS + 1, D, 7), cube(65, D, 8), cube(COLS + 1, D, 9), cube(3, D, 10)
    problems = [(a, a, 1), (b, cube(COLS + 1, D, 11), 0), (c, cube(2 * COLS + 3, D, 12), 0), (d, d, 1), (e, cube(1, D, 13), 0)]
    got = raw(problems)
    assert [g.size for g in got] == [1, ROWS + 1, 65, COLS + 1, 3] and got[0][0] == np.inf
    for g, (q, r, s) in zip(got, problems):
        assert np.array_equal(g, raw([(q, r, s)])[0]) and np.array_equal(g, R.dist2(q, r, self=bool(s)))
    package = S.nn_dist2([(q, None if s else r) for q, r, s in problems])
    assert all(np.array_equal(g, w) for g, w in zip(package, got))
    cross = [(q, r, 0) for q, r, _ in problems]
    zeros, null = raw(cross), raw(cross, self_null=True)
    assert all(np.array_equal(z, n) for z, n in zip(zeros, null)) and zeros[0][0] == 0 and (zeros[3] == 0).all()


def test_edges():
    one = cube(1, 3, 14)
    assert raw([(one, one, 1)])[0].tolist() == [np.inf]
    far_q, far_r = np.full((70, 2), 1e200), np.full((COLS + 5, 2), -1e200)
    with np.errstate(over="ignore"):
        assert np.array_equal(raw([(far_q, far_r, 0)])[0], R.dist2(far_q, far_r)) and (raw([(far_q, far_r, 0)])[0] == np.inf).all()
    same = np.full((ROWS + 9, 4), 0.375)
    assert (raw([(same, same, 1)])[0] == 0).all() and (raw([(same, same[:2], 0)])[0] == 0).all()
    neg = -cube(COLS + 1, 3, 15) * 1e-160                     # squares underflow to 0 and below the normal range: still >= +0
    assert np.array_equal(raw([(neg, neg, 1)])[0], R.dist2(neg, neg, self=True))


def test_refusals_name_the_entry_point_and_leave_the_output_untouched():
    pts = cube(8, 4, 16)
    out = np.full(16, SENTINEL)
    big = MAX_N
    cases = {"D = 0": dict(D=0, q_off=[0, 4], r_off=[0, 4]), "D = 5": dict(D=5, q_off=[0, 4], r_off=[0, 4]),
             "B = 0": dict(D=3, q_off=[0, 4], r_off=[0, 4], B=0), "B above the limit": dict(D=3, q_off=[0, 4], r_off=[0, 4], B=4097),
             "descending queries": dict(D=3, q_off=[0, 4, 3], r_off=[0, 2, 4]), "descending refs": dict(D=3, q_off=[0, 2, 4], r_off=[0, 4, 3]),
             "empty queries": dict(D=3, q_off=[0, 4, 4], r_off=[0, 2, 4]), "empty refs": dict(D=3, q_off=[0, 2, 4], r_off=[0, 0, 4]),
             "offsets not from 0": dict(D=3, q_off=[1, 4], r_off=[0, 4]),
             "a set above the limit": dict(D=1, q_off=[0, big + 1], r_off=[0, 1]),
             "pairs above the cap": dict(D=1, q_off=[0, big], r_off=[0, big])}          # 2^40 pairs; offsets only, no data is read
    for name, kw in cases.items():
        rc, msg = call(kw["D"], kw["q_off"], kw["r_off"], pts, pts, None, out, B=kw.get("B"))
        print("%-24s %d %s" % (name, rc, msg))
        assert rc == 1 and msg.startswith("uda_nn_dist2_np:"), (name, rc, msg)
        assert (out == SENTINEL).all()
    rc, msg = call(3, [0, 4], [0, 4], pts, pts, None, out)      # and the library still works afterwards
    assert rc == 0 and (out[4:] == SENTINEL).all()


def test_kl_goldens_on_the_device():
    """The reference's own KLs at eps=0, bit for bit, +inf (a duplicate inside P), -inf (a point common to P and Q) and nan (both)
    included; many pairs of one dimension in one call give the same."""
    for c in KL_CASES:
        got = S.emp_kl_divergence(GOLD["kl_%s_p" % c], GOLD["kl_%s_q" % c])
        print(c, got, GOLD["kl_%s_exact" % c][0])
        assert np.array_equal([got], GOLD["kl_%s_exact" % c], equal_nan=True)
    d3 = [c for c in KL_CASES if "d3" in c]
    got = S.emp_kl_divergences([(GOLD["kl_%s_p" % c], GOLD["kl_%s_q" % c]) for c in d3])
    assert np.array_equal(got, [GOLD["kl_%s_exact" % c][0] for c in d3], equal_nan=True)
    assert np.isposinf(got[d3.index("d3_dup")]) and np.isneginf(got[d3.index("d3_common")]) and np.isnan(got[d3.index("d3_both")])


def have_scipy():
    try:
        import scipy.stats  # noqa: F401
        return True
    except ImportError:
        return False


def test_jsd_goldens_on_the_device():
    g = lambda c, k: GOLD["jsd_%s_%s" % (c, k)]  # noqa: E731
    got = S.jensen_shannon_from_samples([(g(c, "sp"), g(c, "sq"), g(c, "sm")) for c in JSD_CASES])
    for c, (jsd, kl_pm, kl_qm) in zip(JSD_CASES, got):
        assert np.array_equal([kl_pm, kl_qm], g(c, "kl_exact")) and np.array_equal([jsd], g(c, "jsd_exact"))
    if have_scipy():                                           # with the resampling stage in front
        for c in JSD_CASES:
            assert np.array_equal(S.jensen_shannon_divergences([(g(c, "P"), g(c, "Q"))], int(g(c, "n")[0])), g(c, "jsd_exact"))
            assert S.empirical_jensen_shannon_divergence(g(c, "P"), g(c, "Q"), int(g(c, "n")[0])) == g(c, "jsd_exact")[0]


def test_similarity_table_on_the_device():
    """The reference's table at eps=0: same order, same floats, same flag, nan where a method has no box of a class.  The
    table's resampled sets are not stored (too large), so this needs scipy for the resampling stage."""
    pytest.importorskip("scipy.stats", reason="scipy is not installed: gaussian_kde resampling cannot run")
    classes, methods = [str(c) for c in GOLD["sim_classes"]], [str(m) for m in GOLD["sim_methods"]]
    sets = [{cl: [list(row) for row in GOLD["sim_in_%d_%s" % (s, cl)]] for cl in classes} for s in range(len(methods) + 1)]
    pairs, flag, perclass = S.calculate_set_similarity(sets, classes, methods, return_perclass=True,
                                                       num_samples=int(GOLD["sim_samples"][0]))
    assert [k for k, _ in pairs] == [str(k) for k in GOLD["sim_names_exact"]]
    assert np.array_equal([v for _, v in pairs], GOLD["sim_values_exact"]) and bool(flag) == bool(GOLD["sim_flag_exact"][0])
    assert np.array_equal(np.asarray(perclass), GOLD["sim_perclass_exact"], equal_nan=True) and np.isnan(perclass[2][1])
