"""The Gaussian KDE on the device (`epal.kde_eval_np` / `kde_eval` / `compare_epal` -> `uda_kde_eval_np`; reference
uncertainty_ep_vs_al.py:361-375): the C entry point against the numpy mirror (tests/kde_ref.py) at every size where the tiling
changes (rows per run, points per block, from include/uda_hip.h; work items of one run and of several), ragged batches,
bit-equality of a point wherever it stands, the refusals, and the comparison end to end against what the reference computed (tests/golden/epal_golden.npz).

Tolerance against the mirror: `arg` and the order of summation are identical, so only exp (within an ulp on either side) and the
roundings it perturbs can differ: relative (UDA_KDE_RUN + 64) * 2^-52, plus 1e-300 * sum(w) for points whose terms underflow.
Every test prints the largest ratio of a difference to that bound that it met."""
import os
import re

import numpy as np
import pytest

import kde_ref as R
from uda_amd import capi, epal

pytestmark = pytest.mark.gpu

RUN, POINTS = capi.KDE_RUN, capi.KDE_POINTS
# the number of blocks a call fills before it stops cutting a problem's runs into spans
KDE_BLOCKS = int(re.search(r"static const int kKdeBlocks = (\d+);", open(os.path.join(capi.CSRC, "uda_services.hip")).read()).group(1))
NS = [2, 3, RUN - 1, RUN, RUN + 1, 2 * RUN + 1, 5 * RUN + 7]
MS = [0, 1, POINTS - 1, POINTS, POINTS + 1]
BIG_M = 10000
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epal_golden.npz"))
CLASS_NAMES = [str(c) for c in GOLD["class_names"]]
SENTINEL = -7.0
EPS = 2.0 ** -52


def call(D, data, d_off, weight, points, p_off, out, B=None, device=0):
    lib = capi.load()
    d_off, p_off = np.asarray(d_off, np.int64), np.asarray(p_off, np.int64)
    rc = lib.uda_kde_eval_np(device, D, len(d_off) - 1 if B is None else B, data.ctypes.data, d_off.ctypes.data,
                             None if weight is None else weight.ctypes.data, points.ctypes.data, p_off.ctypes.data, out.ctypes.data)
    return rc, lib.uda_last_error(None).decode()


def raw(problems):
    """One call of the C entry point on [(data [n, D], weight [n] or None, points [m, D])] (weights: all or none): the sums.  The
    output buffer is one element longer than asked for and must keep its sentinel there."""
    D = problems[0][0].shape[1]
    d_off = np.concatenate([[0], np.cumsum([d.shape[0] for d, _, _ in problems])])
    p_off = np.concatenate([[0], np.cumsum([p.shape[0] for _, _, p in problems])])
    data = np.ascontiguousarray(np.concatenate([d for d, _, _ in problems]), np.float64)
    points = np.ascontiguousarray(np.concatenate([p for _, _, p in problems]), np.float64).reshape(-1, D)
    weight = None if problems[0][1] is None else np.ascontiguousarray(np.concatenate([w for _, w, _ in problems]), np.float64)
    out = np.full(int(p_off[-1]) + 1, SENTINEL)
    rc, msg = call(D, data, d_off, weight, points, p_off, out)
    assert rc == 0, msg
    assert out[-1] == SENTINEL
    return [out[a:b] for a, b in zip(p_off[:-1], p_off[1:])]


def ratio(got, want, sum_w):
    """the largest |got - want| over its bound (0 for no points)."""
    bound = (RUN + 64) * EPS * np.abs(want) + 1e-300 * sum_w
    return float(np.max(np.abs(got - want) / bound)) if len(want) else 0.0


def problem(n, m, D, weighted, *seed):
    rng = np.random.default_rng([n, D, int(weighted), *seed])
    data = rng.normal(size=(n, D))
    points = rng.normal(size=(m, D)) * 1.5
    return data, (rng.uniform(0.25, 4.0, n) if weighted else None), points


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_entry_point_equals_the_mirror_at_the_seams(D):
    """Every n of the sweep against every small m, weights NULL and non-uniform, one problem a call; the mirror is taken once per
    (n, weights) on the longest point set - a point's sum does not depend on the points beside it."""
    worst = 0.0
    for n in NS:
        for weighted in (False, True):
            data, w, points = problem(n, MS[-1], D, weighted)
            want = R.kde_sum(data, points, w)
            sum_w = float(n if w is None else w.sum())
            for m in MS:
                got, = raw([(data, w, points[:m])])
                assert got.shape == (m,)
                worst = max(worst, ratio(got, want[:m], sum_w))
                if m == MS[-1]:
                    assert np.all(got > 0) and got.tobytes() == raw([(data, w, points)])[0].tobytes()
    print("D = %d: largest difference / bound = %.4f" % (D, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_a_mesh_of_ten_thousand_points(D, weighted):
    """40 point tiles against every n of the sweep, both weight settings at every D."""
    worst = 0.0
    for n in NS:
        data, w, points = problem(n, BIG_M, D, weighted, 1)
        got, = raw([(data, w, points)])
        worst = max(worst, ratio(got, R.kde_sum(data, points, w), float(w.sum()) if weighted else n))
    print("D = %d, m = %d, weights %s: largest difference / bound = %.4f" % (D, BIG_M, weighted, worst))
    assert worst <= 1.0


def runs_per_item(shapes):
    """The entry point's cut (uda_services.hip), restated: how many runs one work item of each (n, m) problem of a call walks."""
    tiles = sum(-(-m // POINTS) for _, m in shapes)
    want = max(1, -(-KDE_BLOCKS // tiles))
    return [-(-(-(-n // RUN)) // min(-(-n // RUN), want)) for n, _ in shapes]


def scattered(n, distinct, m, D, weighted, *seed):
    """A problem whose m points are `distinct` different ones drawn again and again: the mirror is taken on the different ones
    once - a point's sum does not depend on where it stands - and every repeat must give its bits."""
    data, w, base = problem(n, distinct, D, weighted, *seed)
    idx = np.random.default_rng([m, *seed]).integers(0, distinct, m)
    idx[:distinct] = np.arange(distinct)
    return data, w, base, idx


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape", ["two runs an item, the last one short", "one item walks every run"])
def test_items_that_walk_several_runs(shape, weighted):
    """The calls above cut every problem into items of ONE run (few point tiles, few runs).  A call as large as a real one does
    not: 70 000 rows against a 100 x 100 mesh is 274 runs in items of 6.  Here an item stages a second and a third run in LDS and
    writes their sums: 55 runs against 40 tiles (items of 2, the last item a single short run), and 3 runs against 2 048 tiles,
    where the call stops cutting runs altogether."""
    if shape.startswith("two"):
        n, distinct, m, D, per = 54 * RUN + 1, 1500, BIG_M, 2, 2
    else:
        n, distinct, m, D, per = 2 * RUN + 1, 4096, KDE_BLOCKS * POINTS, 3, 3
    assert runs_per_item([(n, m)]) == [per]
    data, w, base, idx = scattered(n, distinct, m, D, weighted, 5)
    want = R.kde_sum(data, base, w)
    got, = raw([(data, w, base[idx])])
    worst = ratio(got[:distinct], want, float(w.sum()) if weighted else n)
    print("%s, weights %s: largest difference / bound = %.4f" % (shape, weighted, worst))
    assert worst <= 1.0
    assert got.tobytes() == got[:distinct][idx].tobytes()      # every repeat of a point, wherever it stands
    alone, = raw([(data, w, base[:300])])                      # the same points in a call that cuts the runs one by one
    assert runs_per_item([(n, 300)]) == [1] and alone.tobytes() == got[:300].tobytes()


@pytest.mark.parametrize("weighted", [False, True])
def test_a_problem_alone_and_beside_a_large_one_give_the_same_bits(weighted):
    """Alone, the problem is cut into items of one run; beside a problem of 2 048 point tiles one item walks all four of its
    runs.  Same bits, and the large neighbour's own are those of its own call."""
    n, m = 3 * RUN + 5, 700
    data, w, points = problem(n, m, 3, weighted, 6)
    big_d, big_w, big_base, idx = scattered(2, 64, KDE_BLOCKS * POINTS, 3, weighted, 7)
    assert runs_per_item([(n, m)]) == [1] and runs_per_item([(2, len(idx)), (n, m)]) == [1, 4]
    alone, = raw([(data, w, points)])
    big, beside = raw([(big_d, big_w, big_base[idx]), (data, w, points)])
    assert beside.tobytes() == alone.tobytes()
    assert ratio(alone, R.kde_sum(data, points, w), float(w.sum()) if weighted else n) <= 1.0
    assert big.tobytes() == big[:64][idx].tobytes() and ratio(big[:64], R.kde_sum(big_d, big_base, big_w), float(big_w.sum()) if weighted else 2) <= 1.0


def test_terms_that_underflow():
    """A mesh that walks away from the data until every term is 0: the device gives what the mirror gives within the bound and its
    absolute floor, and exactly 0 where nothing is left."""
    data, w, _ = problem(RUN + 1, 0, 2, True, 2)
    t = np.linspace(0, 60, 300)
    points = np.stack([t, -t], 1)
    want = R.kde_sum(data, points, w)
    got, = raw([(data, w, points)])
    assert (want == 0).sum() > 20 and (want > 1e-3).any() and ((want > 0) & (want < 1e-290)).any()
    assert ratio(got, want, float(w.sum())) <= 1.0
    assert (got == 0).sum() > 20


@pytest.mark.parametrize("weighted", [False, True])
def test_a_point_gives_the_same_bits_wherever_it_stands(weighted):
    """A ragged batch of seven problems, one of them without a point: every problem equals its own call bit for bit and the
    mirror within the bound; permuted points give permuted sums."""
    shapes = [(3, 5), (RUN + 1, POINTS + 1), (2 * RUN + 1, 0), (RUN - 1, 1), (5 * RUN + 7, 700), (RUN, POINTS), (2, 300)]
    probs = []
    for k, (n, m) in enumerate(shapes):
        d, w, p = problem(n, m, 3, True, 3, k)
        probs.append((d, w if weighted else None, p))
    batch = raw(probs)
    worst = 0.0
    for (d, w, p), got in zip(probs, batch):
        assert got.shape == (p.shape[0],)
        assert got.tobytes() == raw([(d, w, p)])[0].tobytes()
        worst = max(worst, ratio(got, R.kde_sum(d, p, w), float(d.shape[0] if w is None else w.sum())))
    assert worst <= 1.0
    assert [g.tobytes() for g in raw(probs[::-1])] == [g.tobytes() for g in batch[::-1]]
    d, w, p = probs[4]
    perm = np.random.default_rng(4).permutation(p.shape[0])
    assert raw([(d, w, p[perm])])[0].tobytes() == batch[4][perm].tobytes()
    assert raw([(d, w, p[37:38])])[0].tobytes() == batch[4][37:38].tobytes()
    print("ragged batch: largest difference / bound = %.4f" % worst)


def test_refusals_leave_the_sum_untouched():
    d, p = np.ones((6, 3)), np.zeros((4, 3))
    big = capi.KDE_MAX_PAIRS // 6 + 1
    for D, B, d_off, p_off, text in ((5, 1, [0, 6], [0, 4], "5 coordinates"), (3, 2, [0, 6, 5], [0, 2, 4], "problem 1 descend"),
                                     (3, 2, [0, 3, 6], [0, 4, 2], "problem 1 descend"), (3, 2, [0, 6, 6], [0, 2, 4], "has no data row"),
                                     (3, 1, [0, 6], [0, big], "pairs of a point and a data row")):
        out = np.full(5, SENTINEL)
        rc, msg = call(D, d, d_off, None, p, p_off, out, B=B)
        assert rc == 1 and msg.startswith("uda_kde_eval_np: ") and text in msg, msg
        assert (out == SENTINEL).all()
    with pytest.raises(capi.UdaError, match="uda_kde_eval_np: 5 coordinates"):
        epal.kde_eval_np(5, np.ones((6, 5)), [0, 6], None, np.zeros((4, 5)), [0, 4])


def test_package_equals_scipy_on_the_device():
    from scipy.stats import gaussian_kde
    rng = np.random.default_rng(6)
    sets = [rng.normal(size=(2, 900)) * np.array([[3.0], [0.2]]), rng.normal(size=(2, 40))]
    pts = [rng.normal(size=(2, 500)) * 2, rng.normal(size=(2, 0))]
    w = [rng.uniform(1, 2, 900), None]
    got = epal.kde_eval(sets, pts, w)
    want = gaussian_kde(sets[0], weights=w[0])(pts[0])
    assert np.all(np.abs(got[0] - want) <= (900 + 16) * EPS * want + 1e-300) and got[1].shape == (0,)


@pytest.mark.parametrize("case,k", [(str(case), k) for case in GOLD["cases"] for k in range(len(GOLD["%s_runs" % case]))])
def test_comparison_end_to_end_equals_the_reference(case, k):
    """compare_epal with the device under it: the exact fields are the golden's, the pdf is scipy's within the host tolerance
    (n + 16) * 2^-52, and the mirror's within the device tolerance."""
    uncert, ent, numb = str(GOLD["%s_runs" % case][k]).split("|")
    pre = "%s_r%d_" % (case, k)
    recs = R.golden_case(GOLD, case)
    c = epal.compare_epal(recs, CLASS_NAMES, im_numbs=int(numb), iou_thr=0.1, uncert=uncert, ent=bool(int(ent)))
    assert c.grid_size == int(GOLD[pre + "grid_size"]) and np.array_equal(c.cell_indices, GOLD[pre + "cell_indices"])
    assert np.array_equal(c.hal_lep_ind, GOLD[pre + "hal_lep_ind"]) and np.array_equal(c.lal_hep_ind, GOLD[pre + "lal_hep_ind"])
    for j, data in enumerate(c.metrics):
        for col in (0, 3, 4, 5, 7, 8):
            assert np.array_equal(np.asarray(data[col], np.float64), GOLD["%sm%d_%d" % (pre, j, col)])
    n = int(c.keep.sum())
    want = GOLD[pre + "kde"]
    got = c.pdf.ravel()[::int(GOLD["kde_stride"])]
    assert c.pdf.shape == (100, 100) and np.all(np.abs(got - want) <= (n + 16) * EPS * want + 1e-300)
    host = epal.compare_epal(recs, CLASS_NAMES, im_numbs=int(numb), iou_thr=0.1, uncert=uncert, ent=bool(int(ent)), engine=R.kde_eval_np)
    assert np.all(np.abs(c.pdf - host.pdf) <= (RUN + 64) * EPS * host.pdf + 1e-300)
